"""The convolution at listed cells without a GPU: the ABI of the new entry points and what they refuse before any launch; the integer
logic of vfa_amd/csrc/vfa_cellconv.h (shared host / device code: tap addresses, the zero border, the ownership order of the input
gradient) compiled with g++ into tests/native/cellconv_harness.cpp and checked against a brute-force enumeration of small grids, once
more as a stand-alone program under the host sanitizers; the Python surface (``ops.conv3x3_at_cells``, ``VFANet.heads``)."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import REPO
from native_common import build_harness, run_harness

GXX_FLAGS = ["-O1", "-std=c++17", "-Wall"]
BAD, UNSUPPORTED = 10001, 10002


@pytest.fixture(scope="module")
def built_lib():
    from vfa_amd import build
    return build.build()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "cellconv", "cellconv_harness.cpp", GXX_FLAGS)


@pytest.fixture(scope="module")
def sanitized_harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "cellconv", "cellconv_harness.cpp", GXX_FLAGS, sanitized=True)


def test_entry_points_are_declared_exported_and_bound():
    """Declared, exported, bound, the same number of arguments: tests/test_abi.py, for every symbol.  Here: the cap is one number."""
    text = open(os.path.join(REPO, "include", "vfa_hip.h")).read()
    cap = int(re.search(r"#define\s+VFA_CELLCONV_MAX_ROWS\s+(\d+)", text).group(1))
    shared = open(os.path.join(REPO, "vfa_amd", "csrc", "vfa_cellconv.h")).read()
    assert cap == int(re.search(r"kMaxRows\s*=\s*(\d+)", shared).group(1)) == 1024


def test_the_rotation_rule_is_stated_once():
    """The decode and the new kernels call one device function; neither file restates the arg-max."""
    csrc = os.path.join(REPO, "vfa_amd", "csrc")
    rule = open(os.path.join(csrc, "vfa_rotation.h")).read()
    assert "wave_rotation" in rule and "0.017453292519943295f" in rule and "expf(-x)" in rule
    for name in ("vfa_decode.hip", "vfa_cellconv.hip"):
        text = open(os.path.join(csrc, name)).read()
        assert "vfa_rotation::wave_rotation(" in text and '#include "vfa_rotation.h"' in text, name
        assert "0.017453292519943295f" not in text and "expf(-x)" not in text and "__shfl_xor" not in text, name


def test_refusals_of_the_entry_points(built_lib):
    """What the calls decide before they launch anything (no device is touched: every case returns first)."""
    from vfa_amd import _lib
    lib = _lib.lib()
    assert lib.vfa_conv3x3_at_cells_workspace_bytes(2, 100, 360) == 2 * 100 * 360 * 4
    assert lib.vfa_conv3x3_at_cells_workspace_bytes(0, 100, 360) == 0 and lib.vfa_conv3x3_at_cells_workspace_bytes(2, 0, 360) == 0
    stride = (ctypes.c_longlong * 4)(256 * 16, 16, 4, 1)
    negative = (ctypes.c_longlong * 4)(256 * 16, 16, -4, 1)
    p = ctypes.c_void_p(4096)   # (never dereferenced)

    def fwd(B=1, C=256, L=4, W=4, O=360, k=5, d=4, feat=p, stride=stride, weight=p, cell=p, logits=p, rotation=None, ws=None, ws_bytes=0):
        return lib.vfa_conv3x3_at_cells_f32(feat, stride, weight, cell, B, C, L, W, O, k, d, logits, rotation, ws, ws_bytes, None)

    def bwd(B=1, C=256, L=4, W=4, O=360, k=5, d=4, grad=p, feat=p, stride=stride, weight=p, cell=p, d_feat=p, d_weight=p):
        return lib.vfa_conv3x3_at_cells_backward_f32(grad, feat, stride, weight, cell, B, C, L, W, O, k, d, d_feat, d_weight, None)
    for call in (fwd, bwd):
        assert call(B=-1) == BAD and call(C=0) == BAD and call(L=-1) == BAD and call(W=-1) == BAD and call(O=0) == BAD
        assert call(k=-1) == BAD and call(d=0) == BAD
        assert call(feat=None) == BAD and call(stride=None) == BAD and call(weight=None) == BAD and call(cell=None) == BAD
        assert call(stride=negative) == BAD
        assert call(C=48) == UNSUPPORTED and call(C=16) == UNSUPPORTED and call(weight=ctypes.c_void_p(4100)) == UNSUPPORTED
        assert call(L=1 << 16, W=1 << 16) == UNSUPPORTED
    assert fwd(logits=None, rotation=None) == BAD
    assert fwd(logits=None, rotation=p) == BAD and fwd(logits=None, rotation=p, ws=p, ws_bytes=5 * 360 * 4 - 1) == BAD
    assert fwd(logits=None, rotation=p, ws=ctypes.c_void_p(4098), ws_bytes=1 << 20) == BAD
    assert fwd(B=0) == 0 and fwd(k=0) == 0 and fwd(k=0, C=48) == 0
    assert bwd(grad=None) == BAD and bwd(d_feat=None, d_weight=None) == BAD
    assert bwd(k=1025) == UNSUPPORTED and bwd(k=1025, d_weight=None) == UNSUPPORTED


def test_tap_addresses_against_the_enumeration(harness):
    out = run_harness(harness, "taps")
    taps, outside = (int(v) for v in re.findall(r"(\d+) (?:taps|outside)", out))
    assert taps > 10000 and outside > 1000


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_ownership_order_against_the_enumeration(harness, seed):
    """Cells a dilation apart in a row, a column and a diagonal, duplicates, ids outside the map, and 300 random lists: every touched
    location has exactly one owner, the lowest pair on it, whose walk lists the location's pairs in ascending (row, tap) order."""
    out = run_harness(harness, "owners", str(seed))
    pairs, shared = (int(v) for v in re.findall(r"(\d+) (?:pairs|shared)", out))
    assert pairs > 10000 and shared > 100


def test_integer_logic_under_the_host_sanitizers(sanitized_harness):
    run_harness(sanitized_harness, "taps")
    run_harness(sanitized_harness, "owners", "4")


def _net(mode="3D"):
    from vfa_amd.vfanet import VFANet
    return VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base="resnet18", mode=mode)


def test_heads_and_forward_accept_rotation_at():
    from vfa_amd.vfanet import VFANet
    assert inspect.signature(VFANet.heads).parameters["rotation_at"].default is None
    assert inspect.signature(VFANet.forward).parameters["rotation_at"].default is None
    assert list(inspect.signature(VFANet.detect).parameters) == ["self", "images", "calibs", "grid", "decoder", "cls_thresh"]
    net = _net().eval()
    topdown = torch.randn(1, 256, 8, 8)
    with torch.no_grad():
        dense = net.heads(topdown)
        lazy = net.heads(topdown, rotation_at="detections")
    assert sorted(dense) == ["dim_offset", "heatmap", "loc_offset", "rotation"]
    assert sorted(lazy) == ["dim_offset", "heatmap", "loc_offset", "rotation_head"]
    fused, weight, dilation = lazy["rotation_head"]
    assert tuple(fused.shape) == (1, 256, 8, 8) and weight is net.orient_pred[0].weight and dilation == 4
    for k in ("heatmap", "loc_offset", "dim_offset"):
        assert torch.equal(dense[k], lazy[k]), k
    with pytest.raises(ValueError, match="rotation_at"):
        net.heads(topdown, rotation_at="everywhere")


def test_rotation_at_in_2d_mode_raises():
    net = _net("2D").eval()
    with pytest.raises(ValueError, match="3D"):
        net.heads(torch.randn(1, 256, 8, 8), rotation_at="detections")
    with pytest.raises(ValueError, match="3D"):
        net.heads(torch.randn(1, 256, 8, 8), rotation_at=torch.zeros(1, 3, dtype=torch.int32))


def test_wrapper_refuses_cpu_tensors_and_bad_shapes(built_lib):
    from vfa_amd import ops
    from vfa_amd._lib import VFAHipError
    feat, weight, cells = torch.zeros(1, 32, 4, 4), torch.zeros(5, 32, 3, 3), torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises(VFAHipError):
        ops.conv3x3_at_cells(feat, weight, cells, dilation=4)
    with pytest.raises(VFAHipError):
        _net().eval().heads(torch.randn(1, 256, 8, 8), rotation_at=cells)
    assert list(inspect.signature(ops.conv3x3_at_cells).parameters) == ["feat", "weight", "cells", "dilation", "want_rotation"]
