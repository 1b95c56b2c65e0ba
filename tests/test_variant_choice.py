"""Which instantiation of a fused pass a launch takes: sobfu_amd/csrc/sobfu_variant.hpp, the one place that decides it, through
tests/cpp/variant_tool.cpp (g++, no GPU).  No parity test can see a wrong choice -- every instantiation computes the same bits, a
wrong one is only slower (losing NTBUF costs 3.4 % it/s) -- so the choices are pinned here.

A case line is `A X Y Z compact warp tile` (pass A; tile: the tile kernel), `B X Y Z pX pY pZ compact updates direct long sys apply`
(pass B; long: the longest march is long enough for the halo lead; sys: sys_acquire) or `W X Y Z` (loop_warps_in_pass_a).  The
answer is the kernel's template arguments as 0 / 1 (see the tool) or `refused -3` (SOBFU_E_UNSUPPORTED).  The expected answers were
recorded from the if-ladders in the launchers of solver_kernels.hip that made the choice before the table existed, with their launches
instrumented; they are not derived from the code under test."""
import os
import subprocess

import pytest

KNOBS = ("SOBFU_CACHE_CELLS", "SOBFU_PIPE_B", "SOBFU_WARP_A")

CASES = {
    '': [
        # pass A: every row (non-tile) and the tile kernel
        ('A 256 256 256 1 1 0', 'A 1 1 1'),
        ('A 128 128 128 1 0 0', 'A 1 0 0'),
        ('A 256 256 256 1 0 0', 'A 1 1 0'),
        ('A 256 256 256 0 0 0', 'A 0 0 0'),
        ('A 128 128 128 1 0 1', 'T 1 0 0'),
        ('A 256 256 256 1 0 1', 'T 1 1 0'),
        ('A 256 256 256 0 0 1', 'T 0 0 0'),
        # warp refusals: direct boxes, API format, a resident grid, a volume of 4 GiB or more
        ('A 256 256 256 1 1 1', 'refused -3'),
        ('A 256 256 256 0 1 0', 'refused -3'),
        ('A 128 128 128 1 1 0', 'refused -3'),
        ('A 1024 1024 1024 1 1 0', 'refused -3'),
        # pass B, direct boxes: updates, API / compact outside the own format, the own format at each size
        ('B 256 256 256 256 256 256 1 1 1 0 0 1', 'B 1 1 1 0 0 1 0 0 1'),
        ('B 256 256 256 256 256 256 0 1 1 0 0 1', 'B 1 0 1 0 0 1 0 0 1'),
        ('B 66 66 66 256 256 256 1 0 1 0 0 1', 'B 0 1 1 1 0 0 1 0 1'),
        ('B 256 256 256 256 256 256 1 0 1 0 0 1', 'B 0 1 1 1 0 1 0 1 1'),
        ('B 720 720 720 720 720 720 1 0 1 0 0 1', 'B 0 1 1 1 0 1 0 0 1'),
        ('B 256 256 256 1024 1024 1024 1 0 1 0 0 1', 'B 0 1 1 0 0 1 0 0 1'),
        ('B 256 256 256 256 256 256 0 0 1 0 0 1', 'B 0 0 1 0 0 1 0 0 1'),
        # the same without direct boxes; the halo lead needs long marches
        ('B 256 256 256 256 256 256 1 1 0 1 0 1', 'B 1 1 0 0 0 1 0 0 1'),
        ('B 256 256 256 256 256 256 0 1 0 1 0 1', 'B 1 0 0 0 0 1 0 0 1'),
        ('B 256 256 256 256 256 256 1 0 0 1 0 0', 'B 0 1 0 1 1 1 0 1 0'),
        ('B 256 256 256 256 256 256 1 0 0 0 0 0', 'B 0 1 0 1 0 1 0 1 0'),
        ('B 256 256 256 256 256 256 1 0 0 1 0 1', 'B 0 1 0 1 1 1 0 1 1'),
        ('B 720 720 720 720 720 720 1 0 0 1 0 1', 'B 0 1 0 1 1 1 0 0 1'),
        ('B 128 128 128 128 128 128 1 0 0 1 0 1', 'B 0 1 0 1 0 0 1 0 1'),
        ('B 256 256 256 256 256 256 1 0 0 0 0 1', 'B 0 1 0 1 0 1 0 1 1'),
        ('B 720 720 720 720 720 720 1 0 0 0 0 1', 'B 0 1 0 1 0 1 0 0 1'),
        ('B 256 256 256 1024 1024 1024 1 0 0 1 0 1', 'B 0 1 0 0 0 1 0 0 1'),
        ('B 256 256 256 256 256 256 0 0 0 1 0 1', 'B 0 0 0 0 0 1 0 0 1'),
        # a connected tile (sys_acquire) takes the pipelined march, resident or not
        ('B 66 66 66 256 256 256 1 0 1 0 1 1', 'B 0 1 1 1 0 0 1 0 1'),
        ('B 130 130 130 256 256 256 1 0 0 1 1 1', 'B 0 1 0 1 0 0 1 0 1'),
        ('B 256 256 256 512 512 512 1 0 1 1 1 1', 'B 0 1 1 1 0 1 1 0 1'),
        # refusals: plane of 4 GiB or more; sys_acquire on arrays of 4 GiB or more / without the pipelined march
        ('B 16384 16384 2 16384 16384 2 1 0 0 0 0 1', 'refused -3'),
        ('B 720 720 720 720 720 720 1 0 0 0 1 1', 'refused -3'),
        ('B 256 256 256 256 256 256 0 0 0 0 1 1', 'refused -3'),
        ('B 256 256 256 256 256 256 1 1 0 0 1 1', 'refused -3'),
        ('B 256 256 256 1024 1024 1024 1 0 0 0 1 1', 'refused -3'),
        # !apply: direct boxes, updates, a resident grid, API format, phi_n / arrays of 4 GiB or more, sys_acquire
        ('B 256 256 256 256 256 256 1 0 1 1 0 0', 'refused -3'),
        ('B 256 256 256 256 256 256 1 1 0 1 0 0', 'refused -3'),
        ('B 128 128 128 128 128 128 1 0 0 1 0 0', 'refused -3'),
        ('B 256 256 256 256 256 256 0 0 0 1 0 0', 'refused -3'),
        ('B 256 256 256 1024 1024 1024 1 0 0 1 0 0', 'refused -3'),
        ('B 720 720 720 720 720 720 1 0 0 1 0 0', 'refused -3'),
        ('B 66 66 66 256 256 256 1 0 0 0 1 0', 'refused -3'),
        # the solver's choice
        ('W 128 128 128', 'stream'),
        ('W 256 256 256', 'warp'),
        ('W 512 512 512', 'warp'),
        ('W 720 720 720', 'stream'),
    ],
    'SOBFU_PIPE_B=1': [
        ('B 256 256 256 256 256 256 1 0 1 0 0 1', 'B 0 1 1 1 0 1 1 0 1'),
        ('B 256 256 256 256 256 256 1 0 0 1 0 1', 'B 0 1 0 1 0 1 1 0 1'),
        ('B 256 256 256 256 256 256 1 0 0 1 0 0', 'refused -3'),
        ('W 128 128 128', 'stream'),
        ('W 256 256 256', 'stream'),
        ('W 512 512 512', 'stream'),
    ],
    'SOBFU_PIPE_B=0': [
        ('B 128 128 128 128 128 128 1 0 0 1 0 1', 'B 0 1 0 1 0 0 0 0 1'),
        ('B 66 66 66 256 256 256 1 0 1 0 0 1', 'B 0 1 1 1 0 0 0 0 1'),
        ('B 66 66 66 256 256 256 1 0 1 0 1 1', 'B 0 1 1 1 0 0 1 0 1'),
        ('W 256 256 256', 'warp'),
    ],
    'SOBFU_CACHE_CELLS=0': [
        ('A 128 128 128 1 0 0', 'A 1 1 0'),
        ('A 128 128 128 1 1 0', 'A 1 1 1'),
        ('B 128 128 128 128 128 128 1 0 0 1 0 1', 'B 0 1 0 1 1 1 0 1 1'),
        ('W 128 128 128', 'warp'),
        ('W 256 256 256', 'warp'),
        ('W 512 512 512', 'warp'),
    ],
    'SOBFU_CACHE_CELLS=20000000': [
        ('A 256 256 256 1 0 0', 'A 1 0 0'),
        ('B 256 256 256 256 256 256 1 0 0 1 0 1', 'B 0 1 0 1 0 0 1 0 1'),
        ('W 256 256 256', 'stream'),
    ],
    'SOBFU_WARP_A=0': [
        ('W 128 128 128', 'stream'),
        ('W 256 256 256', 'stream'),
        ('W 512 512 512', 'stream'),
    ],
    'SOBFU_PIPE_B=1 SOBFU_CACHE_CELLS=0': [
        ('W 128 128 128', 'stream'),
        ('W 256 256 256', 'stream'),
    ],
    'SOBFU_PIPE_B=0 SOBFU_CACHE_CELLS=20000000': [
        ('W 256 256 256', 'stream'),
    ],
}


@pytest.fixture(scope="module")
def tool():
    from sobfu_amd import build_host

    return build_host.build_variant_tool()


def run(tool, env, lines):
    e = {k: v for k, v in os.environ.items() if k not in KNOBS}
    e.update(kv.split("=") for kv in env.split())
    r = subprocess.run([tool], input="\n".join(lines) + "\n", capture_output=True, text=True, env=e, timeout=60, check=True)
    return r.stdout.splitlines()


@pytest.mark.parametrize("env", list(CASES))
def test_choice_is_the_ladders(tool, env):
    lines = [c for c, _ in CASES[env]]
    got = run(tool, env, lines)
    assert list(zip(lines, got)) == CASES[env]


def test_every_table_row_is_chosen(tool):
    table = subprocess.run([tool, "--table"], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()
    counts = {k: sum(1 for r in table if r[0] == k) for k in "ATB"}
    assert counts == {"A": 4, "T": 3, "B": 22}  # the instantiations of fused_potential_gradient / tile_potential_gradient / fused_smooth_update_apply
    assert len(set(table)) == len(table)
    chosen = {want for cases in CASES.values() for _, want in cases if want[0] in "ATB"}
    assert chosen == set(table)  # no row is dead, none is missing
