"""Host-only pieces of the neighbourhood and probability verification (no GPU): the numpy restatement against a
brute-force window loop, csim_verify_spatial_finish against the restatement bit for bit (degenerate tables included),
the Brier decomposition, the overflow bound csim_verify_spatial_limit at its edge, the ctypes mirror of
csim_spatial_scores against the C compiler's layout, and the C++ face compiling as plain C++17."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import spatial_restatement as ref
from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALVES = [0, 1, 2, 6]
THR = [0.5, 1.5, 2.5]


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.build()
    return pkg


def integer_case(nx, ny, M=3, seed=0, nan=False):
    rng = np.random.default_rng(seed + 100 * nx + ny)
    x = rng.integers(0, 4, size=(M, ny + 2, nx + 2)).astype(np.float64)
    y = rng.integers(0, 4, size=(ny + 2, nx + 2)).astype(np.float64)
    if nan:
        y[2, 3] = np.nan
        x[1, ny, 1] = np.nan
    return x, y


@pytest.fixture(scope="module", params=[(7, 5), (13, 9)], ids=lambda p: f"{p[0]}x{p[1]}")
def case(request):
    nx, ny = request.param
    x, y = integer_case(nx, ny, nan=True)
    return x, y, ref.restate(x, y, THR, HALVES)


def test_restatement_equals_brute_force(case):
    x, y, r = case
    M = len(x)
    table, nbh, cells, nan_cells = ref.tables(r["n"], r["o"], r["nan"], M, HALVES, window=ref.window_sums_brute)
    assert np.array_equal(table, r["table"]) and np.array_equal(nbh, r["nbh"])
    assert (cells, nan_cells) == (r["cells"], r["nan_cells"]) and nan_cells == 2
    assert cells + nan_cells == (y.shape[0] - 2) * (y.shape[1] - 2)
    for q in range(len(THR)):
        for h in HALVES:
            assert np.array_equal(ref.window_sums(r["n"][q], h), ref.window_sums_brute(r["n"][q], h))
        assert int(table[q].sum()) == cells
    # the brute-force table, cell by cell
    t2 = np.zeros_like(table)
    ny, nx = r["nan"].shape
    for q in range(len(THR)):
        for j in range(ny):
            for i in range(nx):
                if not r["nan"][j, i]:
                    t2[q, r["n"][q, j, i], r["o"][q, j, i]] += 1
    assert np.array_equal(t2, table)


def test_finish_equals_restatement_bit_for_bit(csim, case):
    x, y, r = case
    got = csim.verify_spatial_finish(len(x), r["table"], r["nbh"], r["cells"], r["nan_cells"])
    assert ref.scores_match(got, r["scores"]) == []
    assert (got.cells, got.nan_cells) == (r["cells"], r["nan_cells"])
    assert got.fss.shape == (len(THR), len(HALVES)) and got.hit_rate.shape == (len(THR), len(x) + 1)
    # the ROC ends at (1, 1) and is monotone; a score from real data is a number
    assert np.all(got.hit_rate[:, 0] == 1.0) and np.all(got.false_alarm[:, 0] == 1.0)
    assert np.all(np.diff(got.hit_rate, axis=1) <= 0) and np.all(np.diff(got.false_alarm, axis=1) <= 0)
    assert np.all(np.isfinite(got.brier)) and np.all((got.fss >= 0) & (got.fss <= 1))


def degenerate_tables(M=4, cells=60):
    t = {}
    a = np.zeros((1, M + 1, 2), dtype=np.uint64)
    a[0, :, 0] = [20, 10, 10, 10, 10]                      # the event never happens: SO = 0
    t["no_event"] = a
    b = np.zeros((1, M + 1, 2), dtype=np.uint64)
    b[0, :, 1] = [5, 5, 10, 20, 20]                        # it always happens: SO = n
    t["all_events"] = b
    c = np.zeros((1, M + 1, 2), dtype=np.uint64)
    c[0, 2] = [35, 25]                                     # a single occupied k
    t["one_bin"] = c
    d = np.zeros((1, M + 1, 2), dtype=np.uint64)
    d[0, 0, 0] = cells                                     # nobody exceeds anywhere: S = 0
    t["nothing"] = d
    return t


@pytest.mark.parametrize("name", ["no_event", "all_events", "one_bin", "nothing"])
def test_finish_on_degenerate_tables(csim, name):
    M, cells = 4, 60
    table = degenerate_tables(M, cells)[name]
    assert int(table.sum()) == cells
    # window sums at half = 0 follow from the table; a second scale repeats them
    A = sum(k * k * int(table[0, k].sum()) for k in range(M + 1))
    Bo = int(table[0, :, 1].sum())
    Cc = sum(k * int(table[0, k, 1]) for k in range(M + 1))
    nbh = np.array([[[A, Bo, Cc], [A, Bo, Cc]]], dtype=np.uint64)
    want = ref.finish(M, table, nbh, cells)
    got = csim.verify_spatial_finish(M, table, nbh, cells)
    assert ref.scores_match(got, want) == []
    if name in ("no_event", "all_events"):
        assert np.isnan(got.roc_area[0])
        assert np.all(np.isnan(got.hit_rate if name == "no_event" else got.false_alarm))
        assert not np.any(np.isnan(got.false_alarm if name == "no_event" else got.hit_rate))
        assert got.uncertainty[0] == 0.0 and got.resolution[0] == 0.0
    if name == "one_bin":
        assert got.resolution[0] == 0.0 and got.roc_area[0] == 0.5
    if name == "nothing":
        assert np.all(np.isnan(got.fss)) and got.brier[0] == 0.0
    # no cell at all: every score is NaN
    empty = csim.verify_spatial_finish(M, np.zeros_like(table), np.zeros_like(nbh), 0, 7)
    assert ref.scores_match(empty, ref.finish(M, np.zeros_like(table), np.zeros_like(nbh), 0)) == []
    assert np.isnan(empty.brier[0]) and np.isnan(empty.roc_area[0]) and np.all(np.isnan(empty.fss))
    assert (empty.cells, empty.nan_cells) == (0, 7)


def test_brier_decomposition(csim, case):
    x, y, r = case
    tabs = [r["table"]] + [t for t in degenerate_tables().values()]
    rng = np.random.default_rng(5)
    big = rng.integers(0, 10 ** 9, size=(4, 65, 2)).astype(np.uint64)  # 64 members, a few 10^10 cells
    for table in tabs + [big]:
        M = table.shape[1] - 1
        cells = int(table[0].sum())
        if not all(int(table[q].sum()) == cells for q in range(table.shape[0])):
            table = table[:1]
        got = csim.verify_spatial_finish(M, table, np.zeros((table.shape[0], 0, 3), dtype=np.uint64), cells)
        assert np.all(np.abs(got.brier - (got.reliability - got.resolution + got.uncertainty)) <= 1e-12)


def test_tables_are_consistent_at_half_zero(case):
    x, y, r = case
    M = len(x)
    s = HALVES.index(0)
    for q in range(len(THR)):
        T = r["table"][q].astype(np.int64)
        k = np.arange(M + 1)
        assert int(r["nbh"][q, s, 0]) == int((k * k * T.sum(axis=1)).sum())
        assert int(r["nbh"][q, s, 1]) == int(T[:, 1].sum())
        assert int(r["nbh"][q, s, 2]) == int((k * T[:, 1]).sum())


def test_limit_sits_at_the_bound(csim):
    for M, half in [(2, 0), (5, 2), (64, 32), (64, 31), (63, 8), (1000, 16), (4096, 32), (4096, 0)]:
        w = 2 * half + 1
        most = 2 ** 62 // (M * M * w ** 4)  # the largest nx ny the inequality allows
        nx = min(most, 1000 if most < 10 ** 9 else 2 ** 30)
        ny = most // nx
        assert 1 <= ny < 2 ** 31 - 1
        assert csim.verify_spatial_limit(M, nx, ny, half), (M, half)
        assert not csim.verify_spatial_limit(M, nx, ny + 1, half), (M, half)
        assert M * M * w ** 4 * nx * ny <= 2 ** 62 < M * M * w ** 4 * nx * (ny + 1)
    # what the header says: M = 64 with half = 32 stops just short of 8192^2, half = 31 reaches it
    assert not csim.verify_spatial_limit(64, 8192, 8192, 32) and csim.verify_spatial_limit(64, 8192, 8192, 31)
    assert csim.verify_spatial_limit(64, 7941, 7941, 32) and not csim.verify_spatial_limit(64, 7942, 7942, 32)
    assert csim.verify_spatial_limit(4096, 124, 124, 32) and not csim.verify_spatial_limit(4096, 125, 125, 32)
    assert not csim.verify_spatial_limit(4097, 1, 1, 0)
    for bad in [(0, 4, 4, 0), (3, 0, 4, 0), (3, 4, 0, 0), (3, 4, 4, -1), (3, 4, 4, 33)]:
        with pytest.raises(csim.CsimError) as err:
            csim.verify_spatial_limit(*bad)
        assert err.value.code == 1


def test_finish_and_entry_points_refuse_bad_arguments(csim):
    lib, C = csim.lib(), csim.C
    sc = csim.CsimSpatialScores()
    t = (C.c_ulonglong * 8)()
    assert lib.csim_verify_spatial_finish(0, 1, 0, t, None, 0, 0, C.byref(sc), None, None) == 1
    assert lib.csim_verify_spatial_finish(3, 0, 0, t, None, 0, 0, C.byref(sc), None, None) == 1
    assert lib.csim_verify_spatial_finish(3, 17, 0, t, None, 0, 0, C.byref(sc), None, None) == 1
    assert lib.csim_verify_spatial_finish(3, 1, 9, t, t, 0, 0, C.byref(sc), None, None) == 1
    assert lib.csim_verify_spatial_finish(3, 1, 1, t, None, 0, 0, C.byref(sc), None, None) == 1
    assert lib.csim_verify_spatial_finish(3, 1, 0, None, None, 0, 0, C.byref(sc), None, None) == 1
    assert lib.csim_verify_spatial_finish(3, 1, 0, t, None, 0, 0, None, None, None) == 1
    assert lib.csim_verify_spatial_finish(3, 1, 0, t, None, 0, 0, C.byref(sc), None, None) == 0
    # the compute entry points refuse a null ensemble before anything else
    assert lib.csim_ensemble_verify_spatial(None, None, 0, 1, None, 0, None, None, None, None, None, None, None) == 1
    assert lib.csim_ensemble_verify_spatial_begin(None, None, 0, 1, None, 0, None, 0) == 1
    assert lib.csim_ensemble_verify_spatial_wait(None, None, None, None, None, None, None) == 1


LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "csim.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d %d\n", sizeof(csim_spatial_scores),
           offsetof(csim_spatial_scores, cells), offsetof(csim_spatial_scores, nan_cells),
           offsetof(csim_spatial_scores, brier), offsetof(csim_spatial_scores, reliability),
           offsetof(csim_spatial_scores, resolution), offsetof(csim_spatial_scores, uncertainty),
           offsetof(csim_spatial_scores, roc_area), offsetof(csim_spatial_scores, fss), CSIM_SPATIAL_MAX_HALF,
           CSIM_SPATIAL_MAX_SCALES, CSIM_SPATIAL_MAX_MEMBERS);
    return 0;
}
"""


def test_ctypes_struct_matches_c(csim, tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")
    if cc is None:
        pytest.fail("no C compiler on PATH")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text(LAYOUT)
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-o",
                        str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    S = csim.CsimSpatialScores
    want = [csim.C.sizeof(S)] + [getattr(S, f).offset for f in ("cells", "nan_cells", "brier", "reliability",
                                                                "resolution", "uncertainty", "roc_area", "fss")]
    assert got[:-3] == want
    assert got[-3:] == [csim.SPATIAL_MAX_HALF, csim.SPATIAL_MAX_SCALES, csim.SPATIAL_MAX_MEMBERS]
    assert len(S().fss) == csim.VERIFY_MAX_THRESHOLDS and len(S().fss[0]) == csim.SPATIAL_MAX_SCALES


USE = r"""
#include "climate/ensemble.hpp"

double score(climate::Ensemble& e, const std::vector<double>& truth) {
    climate::SpatialVerification r = e.verify_spatial(truth, {0.5, 1.0}, {0, 2, 8});
    climate::SpatialVerification m = e.verify_spatial_member(0, {0.5});
    e.verify_spatial_begin(truth, {0.5}, {4});
    e.verify_begin(truth, {0.5});
    e.run(20);
    const climate::SpatialVerification w = e.verify_spatial_wait();
    const auto v = e.verify_wait();
    e.verify_spatial_member_begin(1, {0.25}, {1, 3});
    const climate::SpatialVerification u = e.verify_spatial_wait();
    return static_cast<double>(r.table[0] + r.nbh[2] + r.cells + r.nan_cells + m.table.size() + r.forecast) +
           r.scores.fss[1][2] + r.scores.brier[0] + r.scores.reliability[1] + r.scores.resolution[0] +
           r.scores.uncertainty[0] + r.scores.roc_area[0] + r.hit_rate[1] + r.false_alarm[0] + w.scores.fss[0][0] +
           v.scores.crps + u.scores.fss[0][1] + static_cast<double>(climate::verify_spatial_limit(5, 67, 48, 32));
}
"""


def test_cpp_header_compiles(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    src = tmp_path / "use_spatial.cpp"
    src.write_text(USE)
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
