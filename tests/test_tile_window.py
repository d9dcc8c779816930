"""The tap window of a tile of the frame kernels (vfa_amd/csrc/vfa_tile.h, shared host / device code) on the CPU: the C++ harness
tests/native/tile_window_harness.cpp draws random tap bounds (-1 <= coordinate <= size) for the boxes of a tile and checks the
window -- its width, its one or two bands of rows, its slot count, the window row of every image row, the reciprocal of the width the
consumers divide with -- against a brute-force restatement: overlapping, touching and disjoint bands, and tiles without a visible box."""
import pytest

from native_common import build_harness, run_harness


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "tile_window", "tile_window_harness.cpp", ["-O1", "-std=c++17", "-Wall"])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_window_against_brute_force(harness, seed):
    run_harness(harness, str(seed), "4000")
