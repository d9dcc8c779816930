"""The tap window of a tile of the frame kernels (vfa_amd/csrc/vfa_tile.h, shared host / device code) on the CPU: the C++ harness
tests/native/tile_window_harness.cpp draws random tap bounds (-1 <= coordinate <= size) for the boxes of a tile and checks the
window -- its width, its one or two bands of rows, its slot count, the window row of every image row, the reciprocal of the width the
consumers divide with -- against a brute-force restatement: overlapping, touching and disjoint bands, and tiles without a visible box."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tile_window") / "harness")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", exe, os.path.join(REPO, "tests", "native", "tile_window_harness.cpp")])
    return exe


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_window_against_brute_force(harness, seed):
    out = subprocess.run([harness, str(seed), "4000"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("ok"), out.stdout + out.stderr
