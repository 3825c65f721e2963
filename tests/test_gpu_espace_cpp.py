"""The ensemble-space calls through the C++ wrapper (climate::Ensemble::gram, project, transform, eofs and
climate::sym_eigen) on a GPU: driver/test_espace checks that the C++ methods and the C entry points give the same bits on
one 130 x 67 case of 12 forecast members, and what is refused."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRV = os.path.join(ROOT, "climate-sim-mpi-cpp_amd", "driver")


def test_cpp_ensemble_space():
    exe = os.path.join(DRV, "test_espace")
    assert os.path.exists(exe), "driver/test_espace is missing: run __graft_entry__.build()"
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "espace ok" in r.stdout, r.stdout + r.stderr
