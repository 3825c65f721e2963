"""Screening through the C++ wrapper (climate::ObsNetwork::set_active / status / screen_log and the screened
climate::Ensemble::assimilate) on a GPU: driver/test_obsscreen checks that nothing screened gives the unscreened
checksums, that a screened cycle's statuses are csim_obs_screen_decide of the fetched diagnostics and its members those
of the analysis of the used observations, and that the handles survive their ensemble."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "climate-sim-mpi-cpp_amd", "driver")


def test_cpp_obs_screening():
    exe = os.path.join(DRV, "test_obsscreen")
    assert os.path.exists(exe), "driver/test_obsscreen is missing: run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "obsscreen ok" in r.stdout, r.stdout + r.stderr
