"""The LETKF through the C++ wrapper (climate::Ensemble::assimilate_letkf, letkf_info, climate::letkf_nodes and
letkf_blend) on a GPU: driver/test_letkf checks that the C++ methods and the C entry points give the same bits on one
37 x 21 case of 12 forecast members with 40 bilinear observations at spacings 4 and 1, the per-node record, and what is
refused."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "climate-sim-mpi-cpp_amd", "driver")


def test_cpp_letkf():
    exe = os.path.join(DRV, "test_letkf")
    assert os.path.exists(exe), "driver/test_letkf is missing: run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "letkf ok" in r.stdout, r.stdout + r.stderr
