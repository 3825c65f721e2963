"""The ensemble-space dot and the global forecast impact through the C++ wrapper (climate::Ensemble::dot,
climate::Ensemble::obs_impact_global) on a GPU: driver/test_impact_global holds the methods against the C entry points on
a twin, dot of the member fields against gram, and each J_o against csim_obs_impact_global_value on the downloaded
members; a masked observation's +0 and the errors."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "climate-sim-mpi-cpp_amd", "driver")


def test_cpp_impact_global():
    exe = os.path.join(DRV, "test_impact_global")
    assert os.path.exists(exe), "driver/test_impact_global is missing: run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "impact_global ok" in r.stdout, r.stdout + r.stderr
