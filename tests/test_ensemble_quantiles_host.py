"""Host-only pieces of the ensemble quantiles (no GPU): the per-level plan csim_ensemble_quantile_plan must be numpy's
"linear" method, its argument checks, and the C++ face in include/climate/ensemble.hpp compiles as plain C++17."""
import os
import shutil
import subprocess

import numpy as np
import pytest
from numpy.lib import _function_base_impl as nfb

from __graft_entry__ import load_package

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = [0.0, 1.0, 0.5, 1 / 3, 0.1, 0.9, 0.999999, 1e-300]


@pytest.fixture(scope="module")
def csim():
    pkg = load_package()
    pkg.build()
    return pkg


def restated(B, q):
    """the issue's restatement of np.quantile(method="linear")"""
    v = float(B - 1) * q
    if v >= B - 1:
        return B - 1, B - 1, v + 1
    lo = int(np.floor(v))
    return lo, lo + 1, v - lo


def numpy_plan(B, q):
    """numpy's own (previous, next, gamma), indexes -1 read as the last member"""
    qs = np.asarray(q, dtype=np.float64)
    v = nfb._QuantileMethods["linear"]["get_virtual_index"](B, qs)
    prev, nxt = nfb._get_indexes(np.empty(B), v, B)
    gamma = nfb._get_gamma(v, prev, nfb._QuantileMethods["linear"])
    return [int(p) % B for p in prev], [int(n) % B for n in nxt], [float(g) for g in np.atleast_1d(gamma)]


def levels_for(B):
    exact = [k / (B - 1) for k in (1, 2, B // 2, B - 2) if B > 2 and 0 < k < B - 1]
    return LEVELS + exact


@pytest.mark.parametrize("B", list(range(1, 301)) + [4096])
def test_plan_is_numpy_linear(csim, B):
    qs = levels_for(B)
    lo, hi, g = csim.ensemble_quantile_plan(B, qs)
    want = [restated(B, q) for q in qs]
    assert lo == [w[0] for w in want]
    assert hi == [w[1] for w in want]
    assert np.array_equal(np.array(g).view(np.int64), np.array([w[2] for w in want]).view(np.int64))
    nlo, nhi, ng = numpy_plan(B, qs)
    assert (lo, hi) == (nlo, nhi)
    assert np.array_equal(np.array(g).view(np.int64), np.array(ng).view(np.int64))


def test_plan_reproduces_np_quantile(csim):
    rng = np.random.default_rng(5)
    for B in (1, 2, 3, 5, 12, 64, 100, 257):
        x = rng.standard_normal((B, 7))
        x[:, 0] = np.inf
        x[: B // 2, 1] = -np.inf
        s = np.sort(x, axis=0)
        qs = levels_for(B)
        lo, hi, g = csim.ensemble_quantile_plan(B, qs)
        for k, q in enumerate(qs):
            a, b = s[lo[k]], s[hi[k]]
            with np.errstate(invalid="ignore"):
                d = b - a
                got = np.where(g[k] >= 0.5, b - d * (1 - g[k]), a + d * g[k])
                want = np.quantile(x, q, axis=0)
            assert np.array_equal(got, want, equal_nan=True), (B, q)


def test_plan_argument_errors(csim):
    E = csim.CsimError
    for bad in ([-0.1], [1.0000001], [np.nan], [0.5, -np.inf], [np.inf]):
        with pytest.raises(E) as ex:
            csim.ensemble_quantile_plan(10, bad)
        assert ex.value.code == 1, bad
    for bad_members in (0, -3):
        with pytest.raises(E) as ex:
            csim.ensemble_quantile_plan(bad_members, [0.5])
        assert ex.value.code == 1
    with pytest.raises(E) as ex:
        csim.ensemble_quantile_plan(10, [0.5] * 17)  # nq out of range
    assert ex.value.code == 1
    lib, C = csim.lib(), csim.C
    i1, d1 = (C.c_int * 1)(), (C.c_double * 1)(0.5)
    assert lib.csim_ensemble_quantile_plan(10, -1, d1, i1, i1, d1) == 1
    assert lib.csim_ensemble_quantile_plan(10, 1, None, i1, i1, d1) == 1
    assert csim.ensemble_quantile_plan(10, []) == ([], [], [])
    # the full entry point refuses a null ensemble before anything else
    assert lib.csim_ensemble_quantiles(None, 1, d1, 0, None, None, None) == 1
    assert lib.csim_ensemble_quantiles_begin(None, 1, d1, 0, None) == 1
    assert lib.csim_ensemble_quantiles_wait(None, None, None) == 1


USE = r"""
#include "climate/ensemble.hpp"

double bands(climate::Ensemble& e) {
    climate::EnsembleQuantiles r = e.quantiles({0.1, 0.5, 0.9}, {0.0});
    climate::EnsembleQuantiles m = e.quantiles({0.5});
    e.quantiles_begin({0.25, 0.75}, {-1.0, 1.0});
    e.run(20);
    const auto v = e.quantiles_wait();
    const double* q = v.q;
    const double* p = v.exceed;
    e.stats_begin();
    e.quantiles_begin({0.5});
    const auto s = e.stats_wait();
    return r.q[0] + r.exceed[0] + m.q.size() + m.exceed.size() + q[0] + p[0] + v.levels + v.thresholds + s.mean[0] +
           e.quantiles_wait().q[0];
}
"""


def test_cpp_header_compiles(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    src = tmp_path / "use_quantiles.cpp"
    src.write_text(USE)
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
