"""Host-only pieces of the ensemble analysis (no GPU): the Gaspari-Cohn table csim_ensemble_gc_table against an
independent numpy evaluation, the level planner csim_ensemble_assim_plan against a brute-force model of both rules,
its speed on many spread-out observations, argument errors, and the C++ face in include/climate/ensemble.hpp
compiling as plain C++17."""
import os
import shutil
import subprocess
import time

import numpy as np
import pytest

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.build()
    return pkg


# ---- localisation table ------------------------------------------------------------------------------------------

def gc_terms(z):
    """the Gaspari-Cohn polynomial's terms in power form (Gaspari & Cohn 1999, eq. 4.10), per z; their sum is GC(z)"""
    z = np.asarray(z, dtype=np.longdouble)
    inner = np.stack([-z**5 / 4, z**4 / 2, 5 * z**3 / 8, -5 * z**2 / 3, np.zeros_like(z), np.ones_like(z)])
    with np.errstate(divide="ignore"):
        outer = np.stack([z**5 / 12, -z**4 / 2, 5 * z**3 / 8, 5 * z**2 / 3, -5 * z, 4 - 2 / (3 * np.where(z > 0, z, 1))])
    terms = np.where(z <= 1, inner, np.where(z < 2, outer, 0))
    return terms


def half_width(h, loc, n):
    """largest a >= 0 with a * h < 2 loc, by counting, capped at n - 1"""
    a = 0
    while a + 1 <= n - 1 and float(a + 1) * h < 2.0 * loc:
        a += 1
    return a


@pytest.mark.parametrize("dx,dy,loc,nx,ny", [
    (1.0, 1.0, 8.0, 512, 512), (1.0, 2.5, 3.7, 64, 40), (0.3, 0.7, 1.1, 37, 29), (1.0, 1.0, 0.4, 10, 10),
    (2.0, 1.0, 1.0, 5, 1), (1.0, 1.0, 4.0, 8, 8), (0.1, 0.1, 0.35, 100, 3), (1.0, 1.0, 1e6, 9, 6)])
def test_gc_table_against_numpy(csim, dx, dy, loc, nx, ny):
    t = csim.ensemble_gc_table(dx, dy, loc, nx, ny)
    ly, lx = (t.shape[0] - 1) // 2, (t.shape[1] - 1) // 2
    assert lx == half_width(dx, loc, nx) and ly == half_width(dy, loc, ny)
    assert lx <= nx - 1 and ly <= ny - 1
    a = np.arange(-lx, lx + 1, dtype=np.longdouble) * np.longdouble(dx)
    b = np.arange(-ly, ly + 1, dtype=np.longdouble) * np.longdouble(dy)
    z = np.sqrt(a[None, :] ** 2 + b[:, None] ** 2) / np.longdouble(loc)
    terms = gc_terms(z)
    want = np.maximum(terms.sum(axis=0), 0)
    scale = np.abs(terms).sum(axis=0)  # the evaluation's condition: cancellation near z = 2 is in every form
    assert np.all(np.abs(t - want) <= 1e-15 * np.maximum(scale, np.abs(want)) + 1e-300)
    # exact values
    assert t[ly, lx] == 1.0
    assert np.all(t >= 0) and not np.any(np.signbit(t))
    zd = np.sqrt((np.arange(-lx, lx + 1) * dx)[None, :] ** 2 + (np.arange(-ly, ly + 1) * dy)[:, None] ** 2) / loc
    assert np.all(t[zd >= 2] == 0.0)
    assert np.array_equal(t, t[::-1, :]) and np.array_equal(t, t[:, ::-1])


def test_gc_table_caps_and_edges(csim):
    t = csim.ensemble_gc_table(1.0, 1.0, 1e300, 7, 3)
    assert t.shape == (5, 13)
    assert np.all(t == 1.0)  # z rounds to 0 everywhere
    # a * dx == 2c is outside the support: exactly representable boundary
    t = csim.ensemble_gc_table(1.0, 1.0, 2.0, 100, 100)
    assert t.shape == (7, 7)
    t = csim.ensemble_gc_table(1.0, 1.0, 0.5, 100, 100)  # 2c = 1 = dx: only the centre
    assert t.shape == (1, 1) and t[0, 0] == 1.0


def test_gc_table_errors(csim):
    lib, C = csim.lib(), csim.C
    lx, ly = C.c_int(), C.c_int()
    for args in [(0.0, 1.0, 1.0, 4, 4), (1.0, -1.0, 1.0, 4, 4), (1.0, 1.0, 0.0, 4, 4), (1.0, 1.0, float("nan"), 4, 4),
                 (1.0, 1.0, float("inf"), 4, 4), (float("inf"), 1.0, 1.0, 4, 4), (1.0, 1.0, 1.0, 0, 4),
                 (1.0, 1.0, 1.0, 4, 0)]:
        assert lib.csim_ensemble_gc_table(*args, C.byref(lx), C.byref(ly), None) == 1, args
    assert lib.csim_ensemble_gc_table(1.0, 1.0, 1.0, 4, 4, None, C.byref(ly), None) == 1


# ---- planner -----------------------------------------------------------------------------------------------------

def brute_plan(i, j, lx, ly, ordered):
    n = len(i)
    lev = np.zeros(n, dtype=np.int64)
    for o in range(n):
        conf = [p for p in range(o) if abs(int(i[p]) - int(i[o])) <= 2 * lx and abs(int(j[p]) - int(j[o])) <= 2 * ly]
        if ordered:
            lev[o] = 1 + max(lev[p] for p in conf) if conf else 0
        else:
            used = {int(lev[p]) for p in conf}
            L = 0
            while L in used:
                L += 1
            lev[o] = L
    return lev


def obs_sets():
    rng = np.random.default_rng(7)
    sets = []
    # random
    for n, nx, ny in [(200, 64, 64), (300, 37, 29), (50, 5, 1), (120, 256, 256)]:
        sets.append((rng.integers(1, nx + 1, n), rng.integers(1, ny + 1, n), nx, ny))
    # lattice, raster order
    g = np.arange(4, 129, 8)
    I, J = np.meshgrid(g, g)
    sets.append((I.ravel(), J.ravel(), 128, 128))
    # duplicates at one cell, edges and corners
    i = np.array([1, 1, 1, 64, 64, 1, 64, 32, 32, 32, 1, 64, 2, 63])
    j = np.array([1, 1, 1, 64, 64, 64, 1, 1, 64, 32, 32, 32, 1, 64])
    sets.append((i, j, 64, 64))
    return sets


@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("lx,ly", [(0, 0), (1, 2), (8, 8), (3, 0), (16, 5), (200, 200)])
def test_plan_matches_brute_force(csim, ordered, lx, ly):
    for i, j, nx, ny in obs_sets():
        got = csim.ensemble_assim_plan(i, j, lx, ly, ordered=ordered)
        want = brute_plan(i, j, lx, ly, ordered)
        assert np.array_equal(got, want), (ordered, lx, ly, len(i))
        # every conflicting pair in different levels; ordered: in input order
        di = np.abs(i[:, None] - i[None, :]) <= 2 * lx
        dj = np.abs(j[:, None] - j[None, :]) <= 2 * ly
        conf = di & dj & ~np.eye(len(i), dtype=bool)
        assert not np.any(conf & (got[:, None] == got[None, :]))
        if ordered:
            earlier = np.arange(len(i))[:, None] < np.arange(len(i))[None, :]
            rows, cols = np.broadcast_to(got[:, None], conf.shape), np.broadcast_to(got[None, :], conf.shape)
            assert np.all(rows[conf & earlier] < cols[conf & earlier])


def test_plan_level_counts(csim):
    """the issue's figures for a 16-cell lattice over 512^2 with c = 8 cells (lx = ly = 15)"""
    g = np.arange(8, 513, 16)
    I, J = np.meshgrid(g, g)
    lx = csim.ensemble_gc_table(1.0, 1.0, 8.0, 512, 512).shape[1] // 2
    assert lx == 15
    assert csim.ensemble_assim_plan(I.ravel(), J.ravel(), lx, lx).max() + 1 == 4
    assert csim.ensemble_assim_plan(I.ravel(), J.ravel(), lx, lx, ordered=True).max() + 1 == 94


def test_plan_speed(csim):
    rng = np.random.default_rng(3)
    i, j = rng.integers(1, 1025, 65536), rng.integers(1, 1025, 65536)
    for ordered in (False, True):
        t0 = time.perf_counter()
        lev = csim.ensemble_assim_plan(i, j, 15, 15, ordered=ordered)
        dt = time.perf_counter() - t0
        assert dt < 1.0, (ordered, dt)
        assert lev.min() == 0


def test_plan_errors(csim):
    lib, C = csim.lib(), csim.C
    i = (C.c_int * 2)(1, 2)
    lev, nl = (C.c_int * 2)(), C.c_int()
    assert lib.csim_ensemble_assim_plan(-1, i, i, 1, 1, 0, lev, C.byref(nl)) == 1
    assert lib.csim_ensemble_assim_plan(2, None, i, 1, 1, 0, lev, C.byref(nl)) == 1
    assert lib.csim_ensemble_assim_plan(2, i, i, -1, 1, 0, lev, C.byref(nl)) == 1
    assert lib.csim_ensemble_assim_plan(2, i, i, 1, 1, 2, lev, C.byref(nl)) == 1
    assert lib.csim_ensemble_assim_plan(2, i, i, 1, 1, 0, lev, None) == 1
    assert lib.csim_ensemble_assim_plan(2**20 + 1, i, i, 1, 1, 0, lev, C.byref(nl)) == 5  # CSIM_ERR_UNSUPPORTED
    assert lib.csim_ensemble_assim_plan(0, None, None, 1, 1, 0, None, C.byref(nl)) == 0 and nl.value == 0
    # the analysis refuses a null ensemble before anything else
    assert lib.csim_ensemble_assimilate(None, 0, None, None, None, None, 1.0, 1.0, -1, 0, None, None, None, None,
                                        None) == 1


USE = r"""
#include "climate/ensemble.hpp"

double analyse(climate::Ensemble& e) {
    const std::vector<int> i{1, 5}, j{2, 3};
    const std::vector<double> y{0.5, 1.0}, r{0.1, 0.1};
    climate::EnsembleAnalysis a = e.assimilate(i, j, y, r, 4.0, 1.1, 0, true);
    const int nl = e.assimilate_enqueue(i, j, y, r, 4.0);
    e.run(20);
    return a.prior_mean[0] + a.prior_var[1] + a.post_mean[0] + a.post_var[1] + a.nlevels + nl;
}
"""


def test_cpp_header_compiles(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    src = tmp_path / "use_assim.cpp"
    src.write_text(USE)
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_indices_must_be_integral_int32(csim):
    """the Python face refuses indices it cannot pass on exactly, instead of truncating or wrapping them"""
    assert np.array_equal(csim.ensemble_assim_plan([1.0, 40.0], [2.0, 2.0], 3, 3), [0, 0])
    for bad in ([1.5, 2.0], [np.nan, 2.0], [2**32 + 5, 2], [-(2**31) - 1, 2]):
        with pytest.raises(ValueError):
            csim.ensemble_assim_plan(bad, [2, 2], 3, 3)
    with pytest.raises(ValueError):
        csim.ensemble_assim_plan([[1, 2]], [[1, 2]], 3, 3)
