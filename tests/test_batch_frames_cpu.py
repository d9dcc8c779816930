"""Host side of the batched-frame path (no GPU): the new entry points are declared, bound and exported, and the Python layers
validate shapes and route a rig per frame to the frame-by-frame loop."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import REPO

NEW = ["vfa_pipe_batch_workspace_bytes", "vfa_pipe_batch_workspace_layout", "vfa_pipe_batch_records_f32",
       "vfa_pipe_batch_collapse_relu_sum_f32", "vfa_pipe_batch_balance_f32", "vfa_bev_nms_batch_f32"]


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "vfa_hip.h")).read(), flags=re.S)
    return set(re.findall(r"\b(?:int|size_t)\s+(vfa_\w+)\s*\(", text))


def test_batch_entry_points_are_declared_bound_and_exported():
    from vfa_amd import _lib, build
    lib = ctypes.CDLL(build.build())
    declared = _declared()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name


def test_batched_workspace_grows_with_the_batch_and_is_refused_without_frames():
    from vfa_amd import build, ops
    build.build()
    sizes = [ops.pipe_batch_workspace_bytes(b, 7, 40, 64, 5, 3) for b in (1, 2, 4, 8)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    assert ops.pipe_batch_workspace_bytes(0, 7, 40, 64, 5, 3) == 0
    assert ops.pipe_batch_workspace_bytes(1, 7, 40, 64, 5, 3) >= ops.pipe_workspace_bytes(7, 40, 64, 5, 3)
    lay = ops.pipe_batch_workspace_layout(4, 7, 40, 64, 5, 3)
    assert lay["virtual_tiles"] == 4 * lay["tiles_l"] * lay["tiles_w"] and lay["total"] == sizes[2]
    single = ops.pipe_workspace_layout(7, 40, 64, 5, 3)
    assert lay["live"] == single["live"] and lay["shifts"] == single["shifts"]  # (the geometry of the rig, once)


def _mods():
    import vfa_amd
    args = SimpleNamespace(data="MultiviewC", image_size=(720, 1280))
    return [vfa_amd.VFA(256, grid_height=160, cube_size=(25, 25, 32), args=args) for _ in range(3)]


def test_aggregate_frames_validates_shapes_and_an_empty_batch():
    import vfa_amd
    mods = _mods()
    grid = torch.zeros(1, 8, 8, 3)
    lats = [torch.zeros(6, 256, 4, 4)] * 3
    with pytest.raises(ValueError):
        vfa_amd.aggregate_views(*mods, *lats, torch.zeros(3, 3, 4), grid, frames=3)  # 6 maps are not 3 frames of 3 cameras
    with pytest.raises(ValueError):
        vfa_amd.aggregate_views(*mods, *lats, torch.zeros(3, 3, 3, 4), grid, frames=2)  # a rig per frame, but 3 rigs
    empty = vfa_amd.aggregate_views(*mods, *[torch.zeros(0, 256, 4, 4)] * 3, torch.zeros(3, 3, 4), grid, frames=0)
    assert tuple(empty.shape) == (0, 256, 8, 8)


def test_a_rig_per_frame_runs_frame_by_frame(monkeypatch):
    from vfa_amd import aggregate, vfa_op
    mods = _mods()
    grid = torch.zeros(1, 8, 8, 3)
    B, n = 2, 3
    lats = [torch.arange(B * n, dtype=torch.float32).view(B * n, 1, 1, 1).expand(B * n, 256, 4, 4)] * 3
    calibs = torch.arange(B * n * 12, dtype=torch.float32).view(B, n, 3, 4)
    seen = []

    def fake(*a, **k):
        seen.append((a[3][:, 0, 0, 0].tolist(), a[6]))
        return torch.zeros(1, 256, 8, 8)

    monkeypatch.setattr(aggregate, "aggregate_views", fake)
    monkeypatch.setattr(vfa_op, "pipe_frames", lambda *a, **k: pytest.fail("a rig per frame must not take the one-launch path"))
    out = aggregate._aggregate_frames(*mods, *lats, calibs, grid, (-1, 0.95), None, False, None, None, B)
    assert tuple(out.shape) == (B, 256, 8, 8)
    assert [s[0] for s in seen] == [[0.0, 1.0, 2.0], [3.0, 4.0, 5.0]]
    assert all(torch.equal(s[1], calibs[b]) for b, s in enumerate(seen))


def test_vfanet_routes_a_rig_per_frame_to_the_loop(monkeypatch):
    from vfa_amd.vfanet import VFANet
    net = VFANet(SimpleNamespace(data="MultiviewC", image_size=(96, 160)), grid_height=96, cube_size=(50, 50, 32), angle_range=12)
    B, N = 2, 3
    images = torch.zeros(B, N, 3, 96, 160)
    calibs = torch.arange(B * N * 12, dtype=torch.float32).view(B, N, 3, 4)
    grid = torch.zeros(1, 5, 6, 3)
    seen = []
    monkeypatch.setattr(net, "ortho_features", lambda im, c, g, d=False: (seen.append((tuple(im.shape), c)), torch.zeros(1, 256, 5, 6))[1])
    out = net._ortho_frames(images, calibs, grid, False)
    assert tuple(out.shape) == (B, 256, 5, 6) and len(seen) == B
    assert all(s[0] == (N, 3, 96, 160) and torch.equal(s[1], calibs[b]) for b, s in enumerate(seen))
    with pytest.raises(ValueError):
        net._ortho_frames(images, torch.zeros(B, N + 1, 3, 4), grid, False)
