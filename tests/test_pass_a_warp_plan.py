"""The launch plan of pass A's warping march (plan_pass_a_warp, sobfu_amd/csrc/sobfu_geometry.hpp) on the CPU, through
tests/cpp/pass_a_plan_tool.cpp: the plans are the recorded ones (tests/golden/pass_a_warp_plan.tsv: grid, answer), every cell of the
grid is produced by exactly one workgroup, none outside it, and the launch is at most one resident round of the chip (two workgroups
of 16 waves on each of 256 CUs).  The grids are those of tests/test_gpu_pass_a_warp_tiles.py and the two benchmark sizes."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "pass_a_warp_plan.tsv")
GRIDS = ["67 45 37", "130 9 29", "64 17 5", "65 16 3", "70 33 40", "256 256 256", "512 512 512"]
KNOBS = ("SOBFU_ZC_A", "SOBFU_ZC_B", "SOBFU_CACHE_CELLS")


@pytest.fixture(scope="module")
def answers():
    from sobfu_amd import build_host

    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    r = subprocess.run([build_host.build_pass_a_plan_tool()], input="\n".join(GRIDS) + "\n", capture_output=True, text=True, env=env, timeout=120,
                       check=True)
    out = r.stdout.splitlines()
    assert len(out) == len(GRIDS)
    return dict(zip(GRIDS, out))


def test_plans_are_the_recorded_ones(answers):
    with open(GOLDEN) as f:
        golden = dict(line.rstrip("\n").split("\t") for line in f if line.strip())
    assert answers == {g: golden.get(g, "not recorded") for g in GRIDS}


@pytest.mark.parametrize("grid", GRIDS)
def test_every_cell_once_in_one_resident_round(answers, grid):
    m = re.fullmatch(r"ty (\d+) groups (\d+) first [\d ]+(?: \| [\d ]+)+ \| cover min (\d+) max (\d+) outside (\d+)", answers[grid])
    assert m is not None, answers[grid]
    ty, groups, lo, hi, outside = map(int, m.groups())
    assert (lo, hi, outside) == (1, 1, 0)
    assert 0 < groups <= 2 * 256
    assert ty * groups <= 32 * 256  # waves in flight: 8 per SIMD
