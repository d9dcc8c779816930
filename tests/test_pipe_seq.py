"""Step order of the pipelined frame kernel (vfa_amd/csrc/vfa_pipe_seq.h, shared host / device code) on the CPU: the C++
harness tests/native/pipe_seq_harness.cpp enumerates the steps of every workgroup for random live-view masks, layer counts and
work cuts and checks that each (tile, scale, live view, layer, quarter) is visited exactly once, in groups of at most four
views, sets alternating with the step index, with consistent first / last flags."""
import pytest

from native_common import build_harness, run_harness


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "pipe_seq", "pipe_seq_harness.cpp", ["-O1", "-std=c++17"])


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_every_step_once(harness, seed):
    run_harness(harness, str(seed), "400")
