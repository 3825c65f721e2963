"""The ETKF through the C++ wrapper (climate::Ensemble::obs_gram, assimilate_etkf and climate::etkf_weights) on a GPU:
driver/test_etkf checks that the C++ methods and the C entry points give the same bits on one 37 x 21 case of 12
forecast members with 40 bilinear observations, that the analysis is the composition of the public calls, and what is
refused."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "climate-sim-mpi-cpp_amd", "driver")


def test_cpp_etkf():
    exe = os.path.join(DRV, "test_etkf")
    assert os.path.exists(exe), "driver/test_etkf is missing: run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "etkf ok" in r.stdout, r.stdout + r.stderr
