"""Host-only pieces of the ensemble verification (no GPU): the rank histogram's tie-break csim_ensemble_rank_slot against
a numpy restatement of splitmix64's finaliser, the ctypes mirror of csim_verify_scores against the C compiler's layout,
and the C++ face in include/climate/ensemble.hpp compiling as plain C++17."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.build()
    return pkg


def mix(g):
    """splitmix64's finaliser, mod 2^64"""
    z = np.asarray(g, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def test_rank_slot_is_splitmix64(csim):
    gs = [0, 1, 2, 3, 7, 1000, 65535, 2**31 - 1, 2**31, 2**40 + 17, 2**63 - 1, 2**63 - 2, 2**62]
    gs += [int(v) for v in np.random.default_rng(1).integers(0, 2**63 - 1, size=50, dtype=np.int64)]
    with np.errstate(over="ignore"):
        for g in gs:
            for ties in (0, 1, 2, 3, 5, 63, 64, 100, 4095, 4096):
                want = int(mix(g) % np.uint64(ties + 1))
                assert csim.ensemble_rank_slot(g, ties) == want, (g, ties)
    assert csim.ensemble_rank_slot(12345, 0) == 0
    # a known value of the finaliser: splitmix64's first output from seed 0
    with np.errstate(over="ignore"):
        assert int(mix(0)) == 0xE220A8397B1DCDAF


def test_rank_slot_errors(csim):
    lib, C = csim.lib(), csim.C
    v = C.c_int()
    assert lib.csim_ensemble_rank_slot(-1, 3, C.byref(v)) == 1
    assert lib.csim_ensemble_rank_slot(5, -1, C.byref(v)) == 1
    assert lib.csim_ensemble_rank_slot(5, 3, None) == 1
    # the verification entry points refuse a null ensemble before anything else
    assert lib.csim_ensemble_verify(None, None, 0, 0, 0, None, None, None, None, None) == 1
    assert lib.csim_ensemble_verify_begin(None, None, 0, 0, 0, None) == 1
    assert lib.csim_ensemble_verify_wait(None, None, None, None, None) == 1


LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "csim.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %d\n", sizeof(csim_verify_scores), offsetof(csim_verify_scores, cells),
           offsetof(csim_verify_scores, nan_cells), offsetof(csim_verify_scores, crps),
           offsetof(csim_verify_scores, rmse), offsetof(csim_verify_scores, spread),
           offsetof(csim_verify_scores, brier), CSIM_VERIFY_MAX_THRESHOLDS);
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
    S = csim.CsimVerifyScores
    want = [csim.C.sizeof(S)] + [getattr(S, f).offset for f in ("cells", "nan_cells", "crps", "rmse", "spread", "brier")]
    assert got[:-1] == want
    assert got[-1] == csim.VERIFY_MAX_THRESHOLDS == len(S().brier)


USE = r"""
#include "climate/ensemble.hpp"

double score(climate::Ensemble& e, const std::vector<double>& truth) {
    climate::EnsembleVerification r = e.verify(truth, {0.0, 1.0}, true);
    climate::EnsembleVerification m = e.verify_member(0);
    e.verify_begin(truth, {0.5});
    e.run(20);
    const auto v = e.verify_wait();
    e.verify_member_begin(1, {}, false);
    e.quantiles_begin({0.5});
    e.stats_begin();
    const auto s = e.stats_wait();
    const auto w = e.verify_wait();
    const double* q = e.quantiles_wait().q;
    return r.crps[0] + r.brier[1] + static_cast<double>(r.rank_hist[0]) + static_cast<double>(r.scores.cells) +
           r.scores.rmse + m.scores.spread + m.scores.brier[0] + v.crps[0] + v.brier[0] +
           static_cast<double>(v.rank_hist[0] + v.bins + v.thresholds) + v.scores.crps + s.mean[0] + w.scores.crps +
           static_cast<double>(w.scores.nan_cells) + q[0];
}
"""


def test_cpp_header_compiles(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    src = tmp_path / "use_verify.cpp"
    src.write_text(USE)
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
