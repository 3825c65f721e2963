"""The forecast impact through the C++ wrapper (climate::ObsNetwork::impact_capture, climate::Ensemble::obs_impact) on
a GPU: driver/test_obsimpact works the csim.h definition out on the downloaded members with csim_obs_impact_fold and
compares bit for bit, and checks a masked observation's +0, the capture's validity, the errors and a handle that outlives
its ensemble."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "climate-sim-mpi-cpp_amd", "driver")


def test_cpp_obs_impact():
    exe = os.path.join(DRV, "test_obsimpact")
    assert os.path.exists(exe), "driver/test_obsimpact is missing: run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "obsimpact ok" in r.stdout, r.stdout + r.stderr
