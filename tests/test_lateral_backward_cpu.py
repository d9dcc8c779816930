"""The producer's training entry points on a CPU box (declared, exported and bound: tests/test_abi.py): the workspace helper answers
for the bench shapes; host-side argument checks; and VFANet still selects ``laterals()`` in max mode and with the switch off."""
import ctypes
import os

import pytest
import torch


@pytest.fixture(scope="module")
def lib():
    from vfa_amd import build, _lib
    build.build()
    return _lib.lib()


@pytest.mark.parametrize("K,h,w", [(128, 90, 160), (256, 45, 80), (512, 23, 40)])
def test_workspace_helper_answers_for_the_bench_shapes(lib, K, h, w):
    n = 7
    got = lib.vfa_lateral_backward_workspace_bytes(n, K, h, w)
    stats = n * h * 3 * 256 * 8  # the per-row sums alone
    assert got > stats and got % 256 == 0
    assert got < 64 << 20  # (d W partials: a few hundred workgroups of 256 x K floats)
    assert lib.vfa_lateral_backward_workspace_bytes(n, K, h, w) == got  # a function of the shapes alone
    assert lib.vfa_lateral_backward_workspace_bytes(n, 100, h, w) == 0  # K not a multiple of 32
    assert lib.vfa_lateral_backward_workspace_bytes(n, 2048, h, w) == 0  # K > 1024
    assert lib.vfa_lateral_backward_workspace_bytes(-1, K, h, w) == 0


def _arr(n, v=None):
    return (ctypes.c_void_p * n)(*([v] * n))


def test_argument_checks_need_no_device(lib):
    """Bad arguments are refused before anything is launched.  The pointers are fake, so every call also carries a SECOND argument
    that stops it short of any launch -- a zero workspace size, no views, or no output at all --: were the check under test to
    regress, the call would still fail (with another code) instead of reaching the device."""
    fake = 4096
    ks, hw = (ctypes.c_int * 1)(128), (ctypes.c_int * 2)(13, 19)
    need = lib.vfa_lateral_backward_workspace_bytes(1, 128, 13, 19)
    ws_ok, ws_zero = (ctypes.c_size_t * 1)(need), (ctypes.c_size_t * 1)(0)
    full = _arr(1, fake)
    scan = lib.vfa_lateral_scan_backward_f32
    conv = lib.vfa_lateral_conv_backward_f32
    # n_maps outside 1..3 (guard: no workspace)
    assert scan(0, full, full, full, full, full, full, full, full, None, None, None, full, ws_zero, 1, ks, hw, None) == 10001
    assert scan(4, full, full, full, full, full, full, full, full, None, None, None, full, ws_zero, 1, ks, hw, None) == 10001
    # a required pointer missing (guard: no workspace; the convolution call also has no output)
    assert scan(1, _arr(1), full, full, full, full, full, full, full, None, None, None, full, ws_zero, 1, ks, hw, None) == 10001
    assert conv(1, full, full, full, _arr(1), full, None, None, full, ws_zero, 1, ks, hw, None) == 10001
    # K outside the limits (guard: no workspace -> 10001 if the K check were gone)
    bad_k = (ctypes.c_int * 1)(100)
    assert scan(1, full, full, full, full, full, full, full, full, None, None, None, full, ws_zero, 1, bad_k, hw, None) == 10002
    assert conv(1, full, full, full, full, full, None, None, full, ws_zero, 1, (ctypes.c_int * 1)(2048), hw, None) == 10002
    # misaligned d integral / workspace / y (guard: no views -> 0 without a launch if the check were gone)
    assert scan(1, _arr(1, fake + 4), full, full, full, full, full, full, full, None, None, None, full, ws_ok, 0, ks, hw, None) == 10002
    assert scan(1, full, full, full, full, full, full, full, full, None, None, None, _arr(1, fake + 8), ws_ok, 0, ks, hw, None) == 10002
    assert conv(1, full, _arr(1, fake + 4), full, full, full, full, None, full, ws_ok, 0, ks, hw, None) == 10002
    # short workspace (guard: a misaligned d integral, checked after the workspace; the convolution call has no output)
    short = (ctypes.c_size_t * 1)(need - 256)
    assert scan(1, _arr(1, fake + 4), full, full, full, full, full, full, full, None, None, None, full, short, 1, ks, hw, None) == 10001
    assert conv(1, full, full, full, full, full, None, None, full, short, 1, ks, hw, None) == 10001
    # training forward: the statistics outputs are required (guard: K = 100 -> 10002 if that check were gone)
    eps = (ctypes.c_float * 1)(1e-5)
    lsz = (ctypes.c_size_t * 1)(1 << 20)
    assert lib.vfa_lateral_convs_train_f32(1, full, full, full, full, full, eps, full, full, full, None, full, full, lsz, 1, bad_k, hw,
                                           None) == 10001
    assert lib.vfa_lateral_convs_train_f32(1, full, full, full, full, full, eps, full, full, full, full, _arr(1), full, lsz, 1, bad_k,
                                           hw, None) == 10001


def _net(view_reduce="sum"):
    from types import SimpleNamespace
    from vfa_amd.vfanet import VFANet
    torch.manual_seed(0)
    return VFANet(SimpleNamespace(data="MultiviewC", image_size=(64, 96)), grid_height=32, cube_size=(50, 50, 32),
                  angle_range=12, view_reduce=view_reduce)


class _Routed(Exception):
    pass


def _spy_route(monkeypatch, net):
    calls = []

    def route(name):
        def fn(self, images):
            calls.append(name)
            raise _Routed
        return fn
    monkeypatch.setattr(type(net), "laterals", route("laterals"))
    monkeypatch.setattr(type(net), "lateral_integrals", route("integrals"))
    return calls


@pytest.mark.parametrize("on,view_reduce", [(False, "sum"), (True, "max"), (True, "sum")])
def test_vfanet_keeps_laterals_when_the_producer_does_not_train(monkeypatch, on, view_reduce):
    """Switch off, max mode, or CPU tensors: training selects ``laterals()`` as before."""
    from vfa_amd import vfanet, vfa_op
    net = _net(view_reduce)
    monkeypatch.setattr(vfanet, "FUSE_PRODUCER_TRAIN", on)
    monkeypatch.setattr(vfa_op, "producer_train_ok", lambda mods, n: True)
    calls = _spy_route(monkeypatch, net)
    with pytest.raises(_Routed):
        net.ortho_features(torch.rand(2, 3, 64, 96), torch.zeros(2, 3, 4), torch.zeros(1, 4, 4, 3))
    assert calls == ["laterals"]


def test_producer_gate(monkeypatch):
    """``producer_train_ok``: gradients, sum mode, CUDA, cameras and covered modules; the default switch is off."""
    from vfa_amd import vfanet, vfa_op
    assert vfanet.FUSE_PRODUCER_TRAIN == (os.environ.get("VFA_AMD_FUSE_PRODUCER_TRAIN", "0") == "1")
    net = _net()
    monkeypatch.setattr(vfa_op, "producer_train_ok", lambda mods, n: True)

    class FakeCuda:
        is_cuda = True
        shape = (2, 3, 64, 96)
    monkeypatch.setattr(vfanet, "FUSE_PRODUCER_TRAIN", True)
    assert net.producer_train_ok(FakeCuda())
    with torch.no_grad():
        assert not net.producer_train_ok(FakeCuda())
    assert not net.producer_train_ok(torch.rand(2, 3, 64, 96))  # CPU tensors
    net.view_reduce = "max"
    assert not net.producer_train_ok(FakeCuda())
    net.view_reduce = "sum"
    monkeypatch.setattr(vfanet, "FUSE_PRODUCER_TRAIN", False)
    assert not net.producer_train_ok(FakeCuda())


def test_max_mode_still_refuses_integrals():
    import vfa_amd
    from types import SimpleNamespace
    m = [vfa_amd.VFA(256, args=SimpleNamespace(data="MultiviewC", image_size=(64, 96))) for _ in range(3)]
    with pytest.raises(ValueError):
        vfa_amd.aggregate_views(*m, None, None, None, torch.zeros(1, 3, 4), torch.zeros(1, 2, 2, 3), integrals=[torch.zeros(1)] * 3,
                                view_reduce="max")
