"""Max-over-cameras fusion (``view_reduce="max"``) on a box without a GPU: the C ABI and its bindings, the keyword's validation, and the
camera-sharded max of ``_AllReduceMax`` on gloo (world 2 and 3), whose backward must route every element's gradient to the lowest
camera attaining the maximum over ALL ranks -- what ``torch.stack(...).max(0)`` autograd does in one process."""
import os
import re
import socket
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO
from native_common import ABI_VERSION


def test_header_declares_and_python_binds_the_max_entry_points():
    """Declared, exported, bound, the same number of arguments: tests/test_abi.py, for every symbol.  Here: the two numbers of
    arguments themselves, and the header's statement of the ABI version."""
    from vfa_amd import _lib
    assert len(_lib.SIGNATURES["vfa_scale_view_max_f32"]) == 12
    assert len(_lib.SIGNATURES["vfa_scale_view_max_backward_f32"]) == 18
    assert _lib.ABI_VERSION == ABI_VERSION
    assert re.search(rf"#define VFA_ABI_VERSION {ABI_VERSION}\b", open(os.path.join(REPO, "include", "vfa_hip.h")).read())


def test_library_exports_the_max_entry_points():
    import ctypes
    from vfa_amd import build
    lib = ctypes.CDLL(build.build())
    # argument checks come before any device work: they answer on a box without a GPU
    assert lib.vfa_scale_view_max_f32(None, None, None, None, None, None, None, None, 257, ctypes.c_size_t(4), 8, None) == 10001
    assert lib.vfa_scale_view_max_f32(None, None, None, None, None, None, None, None, 2, ctypes.c_size_t(4), 0, None) == 10001
    assert lib.vfa_scale_view_max_f32(None, None, None, None, None, None, None, None, 2, ctypes.c_size_t(4), 8, None) == 10001
    assert lib.vfa_scale_view_max_f32(None, None, None, None, None, None, None, None, 2, ctypes.c_size_t(0), 8, None) == 0
    args = [None] * 14
    assert lib.vfa_scale_view_max_backward_f32(*args, -1, ctypes.c_size_t(4), 8, None) == 10001
    assert lib.vfa_scale_view_max_backward_f32(*args, 3, ctypes.c_size_t(4), 8, None) == 10001


def _mods():
    import vfa_amd
    args = SimpleNamespace(data="MultiviewC", image_size=(720, 1280))
    return [vfa_amd.VFA(4, grid_height=8, cube_size=(25, 25, 32), args=args) for _ in range(3)]


def test_bad_view_reduce_raises_value_error():
    import vfa_amd
    from vfa_amd.vfanet import VFANet
    mods = _mods()
    lat = torch.zeros(1, 4, 6, 8)
    for bad in ("mean", "MAX", None, "min"):
        with pytest.raises(ValueError):
            vfa_amd.aggregate_views(*mods, lat, lat, lat, torch.zeros(1, 3, 4), torch.zeros(1, 2, 2, 3), view_reduce=bad)
        with pytest.raises(ValueError):
            VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), view_reduce=bad)
    with pytest.raises(ValueError):  # max mode takes no integral images
        vfa_amd.aggregate_views(*mods, None, None, None, torch.zeros(1, 3, 4), torch.zeros(1, 2, 2, 3), view_reduce="max",
                                integrals=[torch.zeros(1, 8, 10, 4)] * 3)


def test_view_reduce_is_not_state():
    """The setting is a plain attribute: the state_dict keys stay the reference's in either mode."""
    import json
    from conftest import golden_path
    from vfa_amd.vfanet import VFANet
    args = SimpleNamespace(data="MultiviewC", image_size=(720, 1280))
    net = VFANet(args, view_reduce="max")
    assert net.view_reduce == "max" and VFANet(args).view_reduce == "sum"
    want = [k for k, _, _ in json.load(open(golden_path("vfanet_state_keys.json")))["resnet18_3D"]]
    assert list(net.state_dict().keys()) == want


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _camera_maps(n_cam, M, N):
    """Per-camera maps t_v >= 0 with exact ties planted between cameras of different ranks: rows 0-3 tie cameras 1 and 2 (world 2:
    camera 1 on rank 1, camera 2 on rank 0 -- the lower camera on the higher rank; world 3: ranks 1 and 2), rows 4-7 tie every camera,
    rows 8-11 tie the two highest cameras, row 12 holds zeros everywhere (the n = 0 rank's zeros tie it too)."""
    g = torch.Generator().manual_seed(11)
    t = torch.rand((n_cam, M, N), generator=g, dtype=torch.float32)
    t = torch.floor(t * 64) / 8  # a coarse lattice: many accidental ties on top of the planted ones
    if n_cam >= 3:
        t[1, 0:4] = 100.0
        t[2, 0:4] = 100.0
    t[:, 4:8] = 50.0
    if n_cam >= 2:
        t[n_cam - 2:, 8:12] = 200.0
    t[:, 12] = 0.0
    return t


def _max_worker(rank, world, port, n_cam, out_dir):
    import sys
    sys.path.insert(0, REPO)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from vfa_amd.aggregate import _AllReduceMax, all_reduce_ortho, camera_shard
        M, N = 16, 8
        full = _camera_maps(n_cam, M, N)
        probe = torch.randn((M, N), generator=torch.Generator().manual_seed(5))
        # one process: torch.max(dim=0) autograd over every camera
        ref_t = full.clone().requires_grad_(True)
        ref_y = torch.stack(list(ref_t)).max(0).values
        (ref_y * probe).sum().backward()

        mine = camera_shard(n_cam)
        t = full[mine].clone().requires_grad_(True)
        if mine:
            x, idx = t.max(0)
            argmax = idx.to(torch.uint8)
        else:  # a rank without cameras: zeros, part of the graph
            x = torch.zeros((M, N)).requires_grad_(True)
            argmax = torch.zeros((M, N), dtype=torch.uint8)
        y = _AllReduceMax.apply(x, argmax, len(mine), None)
        assert torch.equal(y, ref_y.detach()), "forward: not the max over all cameras"
        (y * probe).sum().backward()
        if mine:
            assert torch.equal(t.grad, ref_t.grad[mine]), "backward: routed to another camera than torch.max(dim=0)"
            # the planted cross-rank ties went to the lowest camera
            if n_cam >= 3 and 1 in mine:
                assert torch.equal(t.grad[mine.index(1), 0:4], probe[0:4])
            if n_cam >= 3 and 2 in mine:
                assert not t.grad[mine.index(2), 0:4].any()
        else:
            assert not x.grad.any()
        # every camera's gradient, summed over ranks, is the one-process gradient: nothing lost, nothing twice
        total = torch.zeros_like(full)
        if mine:
            total[mine] = t.grad
        dist.all_reduce(total)
        assert torch.equal(total, ref_t.grad)
        # the inference reduction with op=MAX
        part = full[mine].max(0).values if mine else torch.zeros((M, N))
        assert torch.equal(all_reduce_ortho(part.clone(), op=dist.ReduceOp.MAX), ref_y.detach())
        open(os.path.join(out_dir, f"ok{rank}"), "w").write("ok")
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,n_cam", [(2, 5), (3, 7), (3, 2)])
def test_all_reduce_max_routes_like_one_process(world, n_cam, tmp_path):
    port = _free_port()
    mp.spawn(_max_worker, args=(world, port, n_cam, str(tmp_path)), nprocs=world, join=True)
    assert sorted(os.listdir(tmp_path)) == [f"ok{r}" for r in range(world)]
