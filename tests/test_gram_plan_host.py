"""The plan and the lane-to-block geometry of the two Gram sums (csrc/gram_plan.hpp), checked on the CPU:
tools/gram_plan_host_check.cpp runs every cols = 1 .. 257 and every NB through conditions A-E (the block triangle,
ownership, idle waves, the packed triangle, the LDS row), every M = 1 .. 256 and K = 1 .. 16 of the ensemble-space dot's
rectangle through F-H (ownership, idle waves, the LDS rows and size) and the plan against brute force at the cap seams.
No device, no library: the program is the header and the check, compiled here with g++."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "climate-sim-mpi-cpp_amd", "csrc")


def test_gram_plan_host_check(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on PATH")
    exe = tmp_path / "gram_plan_host_check"
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        "-o", str(exe), os.path.join(ROOT, "tools", "gram_plan_host_check.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.rstrip().endswith("gram plan host ok"), r.stdout
