"""Linear observations through the C++ wrapper on a GPU: driver/test_obsop builds a bilinear network from fractional
positions with climate::Ensemble::bilinear_taps, runs one recorded analysis through climate::ObsNetwork, checks the
operator and the diagnostics against a host loop over the downloaded members, and reads the log."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "climate-sim-mpi-cpp_amd", "driver")


def test_cpp_linear_obs_network():
    exe = os.path.join(DRV, "test_obsop")
    assert os.path.exists(exe), "driver/test_obsop is missing: run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "obsop ok" in r.stdout, r.stdout + r.stderr
