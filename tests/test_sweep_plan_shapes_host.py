"""The region tables of the whole-field plans that tests/test_gpu_wide_strip_launch.py counts on, pinned on the CPU:
the two smallest wide plans with a tail (600 x 49181 at seven steps per pass, 618 x 49179 at six, 48-row chunks) and the
flagship launch (16384^2, untuned, at six and seven steps per pass).  Each has all eight regions — left, wide and right
strips of the main part, the same three of the half-height tail, the bottom and the top band — which is every slot of
Tiling::r[8] and the last iteration of the kernel's region decode.  A planner change that drops the tail or a region
from one of these shapes fails here, instead of quietly turning the GPU tests into tests of a simpler launch.  No
device, no library: tools/sweep_plan_print.cpp beside csrc/sweep_plan.cpp, compiled here with g++."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "climate-sim-mpi-cpp_amd", "csrc")

# (nx, ny, T, boundary mix, rows_per_chunk) -> ((nregions, ntiles, tail_blocks, nblocks, rows, nstrips, wide),
#                                               [(t_end, strip0, nstrip, j0, j1, ry, x0, wide) per region])
# div_mode 0 (dx = dy = 1), tuned_rows 0, tail_split 1, wide strips asked for
PINNED = {
    (600, 49181, 7, "dddd", 48): ((8, 4624, 260, 1156, 48, 6, 1), [
        (896, 0, 1, 7, 43014, 48, 0, 0), (2688, 1, 2, 7, 43014, 48, 112, 1), (3584, 3, 1, 7, 43014, 48, 592, 0),
        (3841, 0, 1, 43015, 49175, 24, 0, 0), (4355, 1, 2, 43015, 49175, 24, 112, 1), (4612, 3, 1, 43015, 49175, 24, 592, 0),
        (4618, 0, 6, 1, 6, 6, 0, 0), (4624, 0, 6, 49176, 49181, 6, 0, 0)]),
    (618, 49179, 6, "dddd", 48): ((8, 4544, 240, 1136, 48, 6, 1), [
        (896, 0, 1, 9, 43016, 48, 0, 0), (2688, 1, 2, 9, 43016, 48, 116, 1), (3584, 3, 1, 9, 43016, 48, 604, 0),
        (3821, 0, 1, 43017, 49171, 26, 0, 0), (4295, 1, 2, 43017, 49171, 26, 116, 1), (4532, 3, 1, 43017, 49171, 26, 604, 0),
        (4538, 0, 6, 1, 8, 8, 0, 0), (4544, 0, 6, 49172, 49179, 8, 0, 0)]),
    (16384, 16384, 7, "dddd", 0): ((8, 19544, 1106, 4886, 66, 147, 1), [
        (216, 0, 1, 7, 14262, 66, 0, 0), (14688, 1, 67, 7, 14262, 66, 112, 1), (15120, 68, 2, 7, 14262, 66, 16192, 0),
        (15179, 0, 1, 14263, 16378, 36, 0, 0), (19132, 1, 67, 14263, 16378, 36, 112, 1), (19250, 68, 2, 14263, 16378, 36, 16192, 0),
        (19397, 0, 147, 1, 6, 6, 0, 0), (19544, 0, 147, 16379, 16384, 6, 0, 0)]),
    (16384, 16384, 6, "dddd", 0): ((8, 18707, 1089, 4677, 68, 142, 1), [
        (208, 0, 1, 9, 14152, 68, 0, 0), (13936, 1, 66, 9, 14152, 68, 116, 1), (14352, 67, 2, 9, 14152, 68, 16220, 0),
        (14411, 0, 1, 14153, 16376, 38, 0, 0), (18305, 1, 66, 14153, 16376, 38, 116, 1), (18423, 67, 2, 14153, 16376, 38, 16220, 0),
        (18565, 0, 142, 1, 8, 8, 0, 0), (18707, 0, 142, 16377, 16384, 8, 0, 0)]),
}
# the flagship plan does not depend on the boundary mix of a lone field (the three the GPU test runs)
for _bc in ("nnnn", "dnpd"):
    for _T in (6, 7):
        PINNED[(16384, 16384, _T, _bc, 0)] = PINNED[(16384, 16384, _T, "dddd", 0)]


@pytest.fixture(scope="module")
def printer(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.skip("no g++ on PATH")
    exe = tmp_path_factory.mktemp("sweep_plan") / "sweep_plan_print"
    r = subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                        "-o", str(exe), os.path.join(ROOT, "tools", "sweep_plan_print.cpp"),
                        os.path.join(CSRC, "sweep_plan.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(exe)


def plan(printer, nx, ny, T, bc, rows, wide=1, tuned=0, tail_split=1):
    r = subprocess.run([printer] + [str(v) for v in (nx, ny, T, 0, bc, rows, tuned, tail_split, wide)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    head, regions = None, []
    for ln in r.stdout.splitlines():
        tag, _, rest = ln.partition(":")
        nums = tuple(int(v) for v in rest.split())
        if tag == "plan":
            head = nums
        else:
            assert tag == "region", ln
            regions.append(nums)
    return head, regions


@pytest.mark.parametrize("key", list(PINNED), ids=lambda k: "%dx%d-T%d-%s-r%d" % k)
def test_region_tables_of_the_wide_launch_shapes(printer, key):
    head, regions = plan(printer, *key)
    want_head, want_regions = PINNED[key]
    assert head == want_head, (key, head)
    assert regions == want_regions, (key, regions)
    # what the GPU tests lean on, said once more in words: eight regions, of which the 2nd and 5th are wide, the 4th to 6th
    # are the tail at half height on top of the main part, and the tail's last chunk is ragged in the two small shapes
    assert len(regions) == 8 and [r[7] for r in regions] == [0, 1, 0, 0, 1, 0, 0, 0]
    main, tail = regions[1], regions[4]
    assert tail[3] == main[4] + 1 and tail[5] < main[5] and tail[1:3] == main[1:3] and tail[6] == main[6]
    if key[0] < 1000:
        assert (tail[4] - tail[3] + 1) % tail[5] != 0


def test_the_same_shapes_without_wide_strips_keep_a_tail_but_fewer_regions(printer):
    """the narrow plan of the flagship shape (what a launch without a verdict word gets): main, tail and two bands; the
    two small shapes have too few narrow tiles for a tail (6 strips x 1025 chunks < 8192)"""
    head, regions = plan(printer, 16384, 16384, 7, "dddd", 0, wide=0)
    assert head == (4, 40719, 2242, 10180, 66, 147, 0) and [r[5] for r in regions] == [66, 36, 6, 6]
    head, regions = plan(printer, 600, 49181, 7, "dddd", 48, wide=0)
    assert head[0] == 3 and head[6] == 0 and [r[5] for r in regions] == [48, 6, 6]
