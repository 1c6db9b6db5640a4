"""The lane-to-pixel mapping of the strip kernels that read the soil tables (gcn10::strip_lane_plan of
gcn10_amd/csrc/gcn10_strip_lanes.hpp), walked on the CPU by tests/strip_lane_plan_main.cpp with the kernel's own
arithmetic: every 16-byte vector of a strip is visited exactly once, a thread never changes its column group, the
pieces begin at row boundaries, and a wave spans at most one row end.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (W, rows, grid, slabs, ilp).  B = rows per sub-trip, T = threads of a piece, G = W / 16.
CASES = [
    # the widths of the GPU tests at one workgroup per CU: three full trips and a ragged one per slab at ilp 1
    (1040, 3100, 256, 1, 1), (1040, 3100, 256, 1, 2), (1056, 3100, 256, 1, 1), (1056, 3100, 256, 1, 2),
    (1040, 3100, 197, 1, 4),            # a grid that is no multiple of 8: one piece although slabs are asked for
    (1056, 3100, 256, 0, 2),            # slabs off
    # few rows: fewer than XCDs, one more than XCDs
    (1040, 1, 256, 1, 1), (1040, 7, 256, 1, 2), (1056, 8, 256, 1, 1), (1056, 9, 256, 1, 4), (4096, 1, 1, 1, 1),
    (4096, 5, 13, 1, 2), (4096, 9, 8, 1, 1),
    # ragged last trips: the rows of a piece are no multiple of B * ilp
    (4096, 1001, 64, 1, 2), (4096, 1001, 250, 1, 4), (4096, 333, 21, 0, 1),
    # the benchmark's width, 16 and 8 workgroups per CU
    (36000, 1200, 4096, 1, 2), (36000, 1201, 2048, 1, 4), (36000, 997, 4096, 0, 1),
    # G > T of a slab: the whole grid is one piece
    (36000, 50, 64, 1, 2), (36000, 50, 71, 1, 1),
]
# G > T of the whole grid: no plan, the strip reads the code bytes
NO_PLAN = [(36000, 50, 8, 1, 2), (36000, 3, 5, 0, 1), (16 * (256 * 256 + 1), 3, 256, 1, 2)]


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("lanes") / "strip_lane_plan")
    subprocess.run([cxx, "-std=c++17", "-O2", "-Wall", "-I", os.path.join(ROOT, "gcn10_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tests", "strip_lane_plan_main.cpp")], check=True)
    return exe


def _run(exe, cases):
    args = [str(v) for c in cases for v in c]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = [tuple(int(v) for v in ln.split()) for ln in r.stdout.splitlines()]
    assert [ln[:5] for ln in lines] == [tuple(c) for c in cases]
    return {ln[:5]: dict(pieces=ln[5], B=ln[6], trips=ln[7]) for ln in lines}


def test_every_vector_once_and_every_thread_in_one_column_group(walker):
    got = _run(walker, CASES)
    for c, r in got.items():
        assert r["B"] > 0 and r["trips"] >= 1, c
    # the shapes the cases are there for
    assert got[(1040, 3100, 256, 1, 1)] == dict(pieces=8, B=120, trips=4)      # 388 rows of a slab in trips of 120
    assert got[(1040, 3100, 197, 1, 4)]["pieces"] == 1
    assert got[(1056, 3100, 256, 0, 2)]["pieces"] == 1
    assert got[(36000, 50, 64, 1, 2)] == dict(pieces=1, B=7, trips=4)          # 2048 threads of a slab < 2250 groups
    assert got[(36000, 50, 71, 1, 1)]["pieces"] == 1
    # 131072 threads of an XCD hold 58 rows of 2250 groups; 56 keeps a sub-trip's byte stride a multiple of 128
    assert got[(36000, 1200, 4096, 1, 2)] == dict(pieces=8, B=56, trips=2)
    assert got[(36000, 1201, 2048, 1, 4)]["B"] == 28


def test_no_plan_when_a_row_has_more_groups_than_the_grid_has_threads(walker):
    got = _run(walker, NO_PLAN)
    for c, r in got.items():
        assert r["B"] == 0 and r["trips"] == 0, c
