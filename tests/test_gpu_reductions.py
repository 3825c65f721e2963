"""The reductions of include/csim.h on the GPU (k_reduce<0|1|2> and k_checksum, for one field or one member per
blockIdx.y, and their host folds) at the seams of their loops: widths around one trip of the column loop (255 / 256 / 257),
one row, one column, row counts around one trip of the row loop (1024 blocks; 64 per member in the ensemble), extrema
and differences in the ghost ring, and NaN / Inf as data.

  sum     : bit for bit the numpy restatement of the kernel's order (tests/reduce_restatement.py), and within the
            derived bound gamma_k sum|x| of math.fsum (k = the most additions one value passes through) — a bound of
            the order alone, not a measured tolerance; Inf and NaN are carried.
  minmax  : == the reference's std::min_element / max_element (ora_minmax) over the whole array, ghosts included;
            NaN is skipped (the reference skips it too unless it is element 0), an all-NaN array gives (+inf, -inf).
  linf    : == np.abs(a - b)[1:-1, 1:-1].max(), NaN included: one NaN |a - b| in the interior makes the result NaN.
  checksum: == csim.checksum_host, a function of the interior's bits alone."""
import functools
import math

import numpy as np
import pytest

import reduce_restatement as rr
from __graft_entry__ import load_package
from virtual_ranks import VirtualRanks

pytestmark = pytest.mark.gpu

SHAPE_IDS = [f"{nx}x{ny}" for nx, ny in rr.SHAPES]
ENS_CASES = [(B, nx, ny) for B in rr.ENS_MEMBERS for nx, ny in rr.ENS_SHAPES]
ENS_IDS = [f"B{B}-{nx}x{ny}" for B, nx, ny in ENS_CASES]


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.lib()
    assert pkg.device_count() >= 1, "no GPU visible"
    pkg.set_device(0)
    assert pkg.device_name().startswith("gfx950"), pkg.device_name()
    return pkg


def bits(x):
    return int(np.float64(x).view(np.int64))


@functools.lru_cache(maxsize=None)
def case(nx, ny, cap=rr.CAP_FIELD, seed=0):
    """(field, restated sum, math.fsum, bound) of a shape: computed once, shared, read-only"""
    u = rr.field(nx, ny, seed)
    u.setflags(write=False)
    return u, rr.restated_sum(u, cap), rr.ref_sum(u), rr.sum_bound(u, cap)


def interior_spots(nx, ny, cap=rr.CAP_FIELD):
    spots = dict(rr.positions(nx, ny, cap), **rr.lane_seats(nx, ny))
    return {k: p for k, p in spots.items() if rr.is_interior(p, nx, ny)}


def same_linf(got, want):
    return math.isnan(got) if math.isnan(want) else got == want


# ---- sum -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", rr.SHAPES, ids=SHAPE_IDS)
def test_sum_is_the_restated_order_bit_for_bit(csim, nx, ny):
    u, restated, exact, bound = case(nx, ny)
    f = csim.Field(nx, ny).upload(u)
    s = f.sum()
    print(f"sum {nx}x{ny}: gpu {s!r} restated {restated!r} fsum {exact!r} |gpu - fsum| {abs(s - exact):.3e} "
          f"bound {bound:.3e}")
    assert bits(s) == bits(restated)
    assert abs(s - exact) <= bound
    assert bits(f.sum()) == bits(s)


@pytest.mark.parametrize("nx,ny", rr.SHAPES, ids=SHAPE_IDS)
def test_sum_carries_inf_and_nan_and_leaves_the_ghosts_out(csim, nx, ny):
    u = case(nx, ny)[0]
    f = csim.Field(nx, ny)
    for label, p in interior_spots(nx, ny).items():
        for bad in (np.inf, np.nan):
            v = u.copy()
            v[p] = bad
            s = f.upload(v).sum()
            assert (math.isnan(s) if math.isnan(bad) else s == math.inf), (label, bad, s)
            assert bits(s) == bits(rr.restated_sum(v)) or math.isnan(s)
    # a ring of NaN and Inf around the same interior: the same bits as before
    v = u.copy()
    v[0, :], v[-1, :], v[:, 0], v[:, -1] = np.nan, np.inf, -np.inf, np.nan
    assert bits(f.upload(v).sum()) == bits(case(nx, ny)[1])


# ---- minmax ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", rr.SHAPES, ids=SHAPE_IDS)
def test_minmax_finds_an_extremum_wherever_it_sits(csim, nx, ny):
    u = case(nx, ny)[0]
    f = csim.Field(nx, ny)
    assert f.upload(u).minmax() == rr.ref_minmax(u)
    for label, p in rr.positions(nx, ny).items():
        for planted in (-100.0, 100.0):  # beyond every value of the field, ghosts included
            v = u.copy()
            v[p] = planted
            want = rr.ref_minmax(v)
            assert planted in want
            assert f.upload(v).minmax() == want, (label, planted)
    # +0 and -0 are equal to the reference's comparison: either zero is right
    v = np.zeros_like(u)
    v[rr.positions(nx, ny)["last_row"]] = -0.0
    assert f.upload(v).minmax() == (0.0, 0.0) == rr.ref_minmax(v)


@pytest.mark.parametrize("nx,ny", rr.SHAPES, ids=SHAPE_IDS)
def test_minmax_skips_nan(csim, nx, ny):
    """The contract of include/csim.h: NaN cells are skipped, as the reference's std::min_element skips them
    everywhere but at element 0; an array of nothing but NaN gives (+inf, -inf)."""
    u = case(nx, ny)[0]
    f = csim.Field(nx, ny)
    rng = np.random.default_rng([7, nx, ny])
    v = u.copy()
    v[rng.random(v.shape) < 0.3] = np.nan
    for p in rr.positions(nx, ny).values():
        v[p] = np.nan
    v[0, 0] = u[0, 0]  # element 0 stays a number
    want = rr.ref_minmax(v)
    assert not any(math.isnan(x) for x in want)
    assert f.upload(v).minmax() == want
    # one number among NaN, at element 0 and at the far end
    for p in ((0, 0), (ny + 1, nx + 1)):
        v = np.full_like(u, np.nan)
        v[p] = 2.5
        assert f.upload(v).minmax() == (2.5, 2.5)
    assert f.upload(np.full_like(u, np.nan)).minmax() == (math.inf, -math.inf)
    # infinities are values
    v = u.copy()
    v[0, nx + 1], v[ny, 1] = -np.inf, np.inf
    assert f.upload(v).minmax() == (-math.inf, math.inf) == rr.ref_minmax(v)


# ---- linf_diff -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", rr.SHAPES, ids=SHAPE_IDS)
def test_linf_diff_returns_the_planted_difference(csim, nx, ny):
    u = case(nx, ny)[0]
    a, b = csim.Field(nx, ny).upload(u), csim.Field(nx, ny).upload(u.copy())
    assert bits(a.linf_diff(b)) == bits(0.0)
    for n, (label, p) in enumerate(interior_spots(nx, ny).items()):
        v = u.copy()
        v[p] += 0.125 * (n + 1) * (-1) ** n
        want = rr.ref_linf(u, v)
        assert want == abs(u[p] - v[p]) > 0.0
        assert a.linf_diff(b.upload(v)) == want, label
        assert b.linf_diff(a) == want, label
    # differences in the ghost ring alone do not count
    v = u + 7.0
    v[1:-1, 1:-1] = u[1:-1, 1:-1]
    assert bits(a.linf_diff(b.upload(v))) == bits(0.0)
    # differences everywhere: the maximum, wherever it is
    rng = np.random.default_rng([9, nx, ny])
    v = u + rng.standard_normal(u.shape)
    assert a.linf_diff(b.upload(v)) == rr.ref_linf(u, v)


@pytest.mark.parametrize("nx,ny", rr.SHAPES, ids=SHAPE_IDS)
def test_linf_diff_is_nan_where_a_difference_is(csim, nx, ny):
    """If |a - b| is NaN in an interior cell the result is NaN, whichever lane, wave, block or trip of the row loop
    reads the cell; otherwise it is the maximum, +Inf included.  (An fmax at any stage — lane, wave, block, host —
    drops the NaN: the L-inf of two fields that differ by a NaN was 0.0.)"""
    u = case(nx, ny)[0]
    a, b = csim.Field(nx, ny), csim.Field(nx, ny)
    rng = np.random.default_rng([11, nx, ny])
    noisy = u + rng.standard_normal(u.shape)
    failures = []

    def check(x, y, what):
        got, want = a.upload(x).linf_diff(b.upload(y)), rr.ref_linf(x, y)
        print(f"linf {nx}x{ny} {what}: gpu {got!r} numpy {want!r}")
        if not same_linf(got, want):
            failures.append((what, got, want))
        return want

    for label, p in interior_spots(nx, ny).items():
        v = u.copy()
        v[p] = np.nan
        assert math.isnan(check(u, v, f"NaN in b only, the only differing cell, at {label}"))
        assert math.isnan(check(v, u, f"NaN in a only, the only differing cell, at {label}"))
        assert math.isnan(check(v, v.copy(), f"NaN in both at {label}"))
        w = noisy.copy()
        w[p] = np.nan
        assert math.isnan(check(u, w, f"NaN in b among finite differences at {label}"))
        v = u.copy()
        v[p] = np.inf
        assert math.isnan(check(v, v.copy(), f"+Inf in both at {label}"))
        assert check(u, v, f"+Inf in b only at {label}") == math.inf
        v[p] = -np.inf
        assert check(noisy, v, f"-Inf in b among finite differences at {label}") == math.inf
    # non-finite ghosts change nothing
    v = u.copy()
    v[0, :], v[-1, :], v[:, 0], v[:, -1] = np.nan, np.inf, -np.inf, np.nan
    assert check(u, v, "NaN and Inf in the ghost ring only") == 0.0
    assert not failures, failures


# ---- the stepper's entry points ----------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", [(513, 62), (67, 2051)], ids=["513x62-one-trip", "67x2051-three-trips"])
def test_stepper_reductions_equal_the_fields(csim, nx, ny):
    u, restated, _, _ = case(nx, ny)
    f = csim.Field(nx, ny).upload(u)
    st = csim.Stepper.single(nx, ny)
    st.upload(u)
    try:
        got, want = st.minmax(), f.minmax()
        assert (bits(got[0]), bits(got[1])) == (bits(want[0]), bits(want[1])) and got == rr.ref_minmax(u)
        assert bits(st.sum()) == bits(f.sum()) == bits(restated)
        assert st.checksum() == csim.checksum_host(u[1:-1, 1:-1])
    finally:
        st.close()


# ---- checksum --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nx,ny", rr.SHAPES, ids=SHAPE_IDS)
def test_checksum_is_a_function_of_the_interiors_bits(csim, nx, ny):
    u = case(nx, ny)[0]
    st = csim.Stepper.single(nx, ny)

    def checksum(x):
        st.upload(x)
        return st.checksum()

    try:
        base = checksum(u)
        assert base == csim.checksum_host(u[1:-1, 1:-1])
        for label, p in interior_spots(nx, ny).items():
            v = u.copy()
            v[p] = 0.0
            plus = checksum(v)
            v[p] = -0.0
            minus = checksum(v)
            assert minus == csim.checksum_host(v[1:-1, 1:-1]), label
            assert len({base, plus, minus}) == 3, label
            sums = []
            for payload in (0x7FF8000000000000, 0x7FF8000000000001):
                v.view(np.uint64)[p] = payload
                sums.append(checksum(v))
                assert sums[-1] == csim.checksum_host(v[1:-1, 1:-1]), (label, hex(payload))
            assert sums[0] != sums[1] and base not in sums, label
        # the ghost ring is not in it
        v = u + 1.0
        v[1:-1, 1:-1] = u[1:-1, 1:-1]
        assert checksum(v) == base
        v[0, :], v[-1, :], v[:, 0], v[:, -1] = np.nan, np.inf, -0.0, 1e300
        assert checksum(v) == base
    finally:
        st.close()


# ---- ensemble --------------------------------------------------------------------------------------------------

def ens_fields(B, nx, ny):
    return np.stack([case(nx, ny, rr.CAP_ENSEMBLE, seed=100 + m)[0] for m in range(B)])


def per_member_spots(B, nx, ny, interior=False):
    """for every member another spot of the list, so that a partial read from the wrong member shows"""
    spots = interior_spots(nx, ny, rr.CAP_ENSEMBLE) if interior else rr.positions(nx, ny, rr.CAP_ENSEMBLE)
    spots = list(spots.items())
    return [[spots[(r + 2 * m) % len(spots)] for m in range(B)] for r in range(len(spots))]


@pytest.mark.parametrize("B,nx,ny", ENS_CASES, ids=ENS_IDS)
def test_ensemble_minmax_per_member(csim, B, nx, ny):
    X = ens_fields(B, nx, ny)
    e = csim.Ensemble(B, nx, ny)
    try:
        e.upload_all(X)
        assert np.array_equal(e.minmax(), np.array([rr.ref_minmax(x) for x in X]))
        for sign in (-1.0, 1.0):
            for rnd in per_member_spots(B, nx, ny):
                Y = X.copy()
                for m, (label, p) in enumerate(rnd):
                    Y[m][p] = sign * (100.0 + m)  # another value in another place in every member
                e.upload_all(Y)
                want = np.array([rr.ref_minmax(y) for y in Y])
                assert np.array_equal(want[:, 0 if sign < 0 else 1], sign * (100.0 + np.arange(B)))
                assert np.array_equal(e.minmax(), want), [label for label, _ in rnd]
        # NaN is skipped; a member of nothing but NaN gives (+inf, -inf) and leaves the others alone
        rng = np.random.default_rng([13, B, nx, ny])
        Y = X.copy()
        Y[rng.random(Y.shape) < 0.3] = np.nan
        Y[:, 0, 0] = X[:, 0, 0]
        e.upload_all(Y)
        want = np.array([rr.ref_minmax(y) for y in Y])
        assert not np.isnan(want).any() and np.array_equal(e.minmax(), want)
        Y[B - 1] = np.nan
        e.upload_all(Y)
        want[B - 1] = (math.inf, -math.inf)
        assert np.array_equal(e.minmax(), want)
    finally:
        e.close()


@pytest.mark.parametrize("B,nx,ny", ENS_CASES, ids=ENS_IDS)
def test_ensemble_sums_and_checksums_per_member(csim, B, nx, ny):
    X = ens_fields(B, nx, ny)
    cases = [case(nx, ny, rr.CAP_ENSEMBLE, seed=100 + m) for m in range(B)]
    e = csim.Ensemble(B, nx, ny)
    try:
        e.upload_all(X)
        s = e.sums()
        for m, (_, restated, exact, bound) in enumerate(cases):
            print(f"ensemble sum B{B} {nx}x{ny} member {m}: gpu {s[m]!r} restated {restated!r} fsum {exact!r} "
                  f"|gpu - fsum| {abs(s[m] - exact):.3e} bound {bound:.3e}")
            assert bits(s[m]) == bits(restated)
            assert abs(s[m] - exact) <= bound
        assert np.array_equal(e.sums().view(np.int64), s.view(np.int64))
        assert e.checksums() == [csim.checksum_host(x[1:-1, 1:-1]) for x in X]
        # Inf in one member, NaN in another (or the same, when there is one): each member's own result
        for r, rnd in enumerate(per_member_spots(B, nx, ny, interior=True)):
            Y = X.copy()
            for m, (label, p) in enumerate(rnd):
                Y[m][p] = (np.inf, np.nan, 3.0)[(m + r) % 3]
            e.upload_all(Y)
            got, want = e.sums(), np.array([rr.restated_sum(y, rr.CAP_ENSEMBLE) for y in Y])
            assert np.array_equal(np.isnan(got), np.isnan(want)), [label for label, _ in rnd]
            ok = ~np.isnan(want)
            assert np.array_equal(got[ok].view(np.int64), want[ok].view(np.int64)), [label for label, _ in rnd]
            assert e.checksums() == [csim.checksum_host(y[1:-1, 1:-1]) for y in Y]
        # the ghosts are in neither
        Y = X + 1.0
        Y[:, 1:-1, 1:-1] = X[:, 1:-1, 1:-1]
        e.upload_all(Y)
        assert np.array_equal(e.sums().view(np.int64), s.view(np.int64))
        assert e.checksums() == [csim.checksum_host(x[1:-1, 1:-1]) for x in X]
    finally:
        e.close()


# ---- one kernel, two kinds of offsets: a rank's global position and a member's slab ------------------------------

def test_checksum_follows_the_global_offsets_of_a_decomposition(csim):
    """Four ranks of a 61 x 29 field: every rank's checksum is checksum_host of its tile at its global offsets, and the
    four add up (mod 2^64) to the checksum of the whole interior; again with a -0.0 in the tile of rank 3."""
    nxg, nyg, world = 61, 29, 4
    u = rr.field(nxg, nyg)
    vr = VirtualRanks(csim, world, nxg, nyg)
    try:
        assert any(d.x_offset > 0 for d in vr.decs) and any(d.y_offset > 0 for d in vr.decs)
        d3 = vr.decs[3]
        spot = (1 + d3.y_offset + d3.ny_local // 2, 1 + d3.x_offset + d3.nx_local // 2)  # array position in u
        seen = []
        for planted in (None, -0.0):
            v = u.copy()
            if planted is not None:
                v[spot] = planted
            # tiles cut with their ring of neighbouring values: the ghosts are not zero and not in the checksum
            vr.upload_tiles(lambda r, d: v[d.y_offset:d.y_offset + d.ny_local + 2,
                                           d.x_offset:d.x_offset + d.nx_local + 2].copy())
            per_rank = [st.checksum() for st in vr.st]
            for r, d in enumerate(vr.decs):
                tile = v[1 + d.y_offset:1 + d.y_offset + d.ny_local, 1 + d.x_offset:1 + d.x_offset + d.nx_local]
                assert per_rank[r] == csim.checksum_host(tile, d.x_offset, d.y_offset, nxg), (r, planted)
            whole = csim.checksum_host(v[1:-1, 1:-1])
            assert sum(per_rank) % (1 << 64) == whole == vr.checksum(), planted
            seen.append((whole, per_rank))
        assert seen[0][0] != seen[1][0] and seen[0][1][:3] == seen[1][1][:3] and seen[0][1][3] != seen[1][1][3]
    finally:
        vr.close()


def test_a_member_reduces_as_the_stepper_that_holds_the_same_field(csim):
    """Member 1 of three 257 x 65 members against a Stepper of the same array: the same checksum and min / max; each
    sum is its own cap's restated order bit for bit (65 rows: 64 blocks in the ensemble, 65 in the Stepper), so the two
    sums differ by no more than the two orders' bounds against the exact sum together."""
    B, nx, ny = 3, 257, 65
    X = ens_fields(B, nx, ny)
    u = X[1]
    e, st = csim.Ensemble(B, nx, ny), csim.Stepper.single(nx, ny)
    try:
        e.upload_all(X)
        st.upload(u)
        assert e.checksums()[1] == st.checksum() == csim.checksum_host(u[1:-1, 1:-1])
        got, want = e.minmax()[1], st.minmax()
        assert (bits(got[0]), bits(got[1])) == (bits(want[0]), bits(want[1])) and want == rr.ref_minmax(u)
        se, ss = e.sums()[1], st.sum()
        print(f"sum 257x65: member {se!r} stepper {ss!r}")
        assert bits(se) == bits(rr.restated_sum(u, rr.CAP_ENSEMBLE))
        assert bits(ss) == bits(rr.restated_sum(u, rr.CAP_FIELD))
        assert abs(se - ss) <= rr.sum_bound(u, rr.CAP_ENSEMBLE) + rr.sum_bound(u, rr.CAP_FIELD)
    finally:
        e.close()
        st.close()
