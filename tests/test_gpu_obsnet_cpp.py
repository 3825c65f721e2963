"""climate::ObsNetwork, the C++ wrapper of the observation networks, on a GPU: driver/test_obsnet compares the analysis
through a network with Ensemble::assimilate bit for bit, reads the log and the diagnostics back, and lets networks
outlive their ensemble (the handle they share with it is emptied, so destroying or moving them is safe and every
other call throws)."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "climate-sim-mpi-cpp_amd", "driver")


def test_cpp_obs_network():
    exe = os.path.join(DRV, "test_obsnet")
    assert os.path.exists(exe), "driver/test_obsnet is missing: run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "obsnet ok" in r.stdout, r.stdout + r.stderr
