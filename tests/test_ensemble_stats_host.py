"""The C++ face of the ensemble statistics (climate::Ensemble::stats / stats_begin / stats_wait in
include/climate/ensemble.hpp) compiles as plain C++17 against the public headers, without HIP."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

USE = r"""
#include "climate/ensemble.hpp"

double spread(climate::Ensemble& e) {
    const int bc[4] = {CSIM_BC_DIRICHLET, CSIM_BC_NEUMANN, CSIM_BC_PERIODIC, CSIM_BC_DIRICHLET};
    climate::Ensemble other(4, 16, 8, 1.0, 1.0, bc);
    climate::EnsembleStats s = e.stats();
    climate::EnsembleStats p = other.stats(0);
    e.stats_begin();
    other.stats_begin(0);
    e.run(20);
    const auto v = e.stats_wait();
    const double* mean = v.mean;
    const double* var = v.var;
    const double* lo = v.min;
    const double* hi = v.max;
    return s.mean[0] + s.var[0] + s.min[0] + s.max[0] + p.var.size() + mean[0] + var[0] + lo[0] + hi[0] +
           other.stats_wait().var[0];
}
"""


def test_cpp_header_compiles(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no C++ compiler on PATH")
    src = tmp_path / "use_stats.cpp"
    src.write_text(USE)
    r = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
