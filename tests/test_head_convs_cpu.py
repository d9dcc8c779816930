"""The heads' dense 3x3 convolutions without a GPU: the integer rules of vfa_amd/csrc/vfa_conv.h (shared host / device code) compiled
with g++ into tests/native/conv_harness.cpp and checked against brute force, once more as a stand-alone program under the host
sanitizers; the numpy restatement of the kernels' arithmetic (tests/conv_common.py) against the two yardsticks, with the restatement
that drops the lo pieces failing (N); what the entry points refuse before they launch; the Python surface."""
import ctypes
import inspect
import re
from types import SimpleNamespace

import pytest
import torch

import conv_common as cc
from native_common import build_harness, run_harness

GXX_FLAGS = ["-O1", "-std=c++17", "-Wall"]
BAD, UNSUPPORTED = 10001, 10002


@pytest.fixture(scope="module")
def built_lib():
    from vfa_amd import build
    return build.build()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "conv", "conv_harness.cpp", GXX_FLAGS)


@pytest.fixture(scope="module")
def sanitized_harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "conv", "conv_harness.cpp", GXX_FLAGS, sanitized=True)


def test_tiles_windows_and_taps_against_the_enumeration(harness):
    out = run_harness(harness, "tiles")
    cells, taps, outside, locations = (int(v) for v in re.findall(r"(\d+) (?:cells|taps|outside|locations)", out))
    assert cells > 100000 and taps > 1000000 and outside > 100000 and locations > 100000


def test_packed_weight_index_is_a_bijection(harness):
    out = run_harness(harness, "weights")
    assert int(re.search(r"(\d+) weights", out).group(1)) > 1000000


def test_integer_rules_under_the_host_sanitizers(sanitized_harness):
    run_harness(sanitized_harness, "tiles")
    run_harness(sanitized_harness, "weights")


@pytest.mark.parametrize("C,O,L,W,d", [(32, 5, 9, 11, 1), (256, 4, 9, 11, 2), (256, 3, 6, 7, 4)])
def test_restated_dense_arithmetic_meets_both_yardsticks_and_dropping_lo_fails(C, O, L, W, d):
    x, w = cc.inputs(2, C, O, L, W, seed=C + d)
    y64, y32 = cc.conv64(x, w, d), cc.conv32(x, w, d)
    y = cc.emulate_dense(x, w, d)
    cc.check_elementwise(y, x, w, d, cc.n_dense(C), "restated dense")
    cc.check_normwise(y, y64, y32, "restated dense")
    coarse = cc.emulate_dense(x, w, d, drop_lo=True)
    assert cc.normwise(coarse, y64) > 1e-4                      # an fp16 product: three orders of magnitude off
    with pytest.raises(AssertionError, match=r"\(N\)"):
        cc.check_normwise(coarse, y64, y32, "hi pieces alone")


def test_restated_dense_arithmetic_is_per_frame():
    """A frame's scale comes from that frame: the bits of a frame alone and in a batch whose other frame is 1000 times larger."""
    x, w = cc.inputs(2, 32, 3, 5, 6, seed=3)
    x[1] *= 1000.0
    assert torch.equal(cc.emulate_dense(x, w, 1)[0], cc.emulate_dense(x[:1], w, 1)[0])


@pytest.mark.parametrize("C,O,d,prologue", [(32, 3, 1, False), (256, 1, 4, False), (256, 2, 1, True)])
def test_restated_few_output_arithmetic_meets_both_yardsticks(C, O, d, prologue):
    x, w = cc.inputs(2, C, O, 7, 9, seed=7 * C + d)
    affine, xp64, xp32 = None, x, x
    if prologue:
        gen = torch.Generator().manual_seed(1)
        affine = (torch.rand(2, C, generator=gen) + 0.5, torch.randn(2, C, generator=gen))
        xp64 = torch.relu(affine[0].double()[:, :, None, None] * x.double() + affine[1].double()[:, :, None, None])
        xp32 = torch.relu(affine[0][:, :, None, None] * x + affine[1][:, :, None, None])   # (as the library chain does it)
    y = cc.emulate_few(x, w, d, affine)
    cc.check_elementwise(y, xp64, w, d, cc.n_few(C), "restated few")   # (the prologue is one fmaf: one of the four spare u)
    cc.check_normwise(y, cc.conv64(xp64, w, d), cc.conv32(xp32, w, d), "restated few")


def test_refusals_of_the_entry_points(built_lib):
    """What the calls decide before they launch anything (no device is touched: every case returns first)."""
    from vfa_amd import _lib
    lib = _lib.lib()
    assert lib.vfa_conv3x3_packed_bytes(256, 256) == 64 + 256 * 256 * 9 * 2 * 2
    assert lib.vfa_conv3x3_packed_bytes(1, 32) == 64 + 128 * 32 * 9 * 2 * 2          # outputs are padded to the tile
    assert lib.vfa_conv3x3_packed_bytes(256, 48) == 0 and lib.vfa_conv3x3_packed_bytes(0, 32) == 0
    assert lib.vfa_conv3x3_workspace_bytes(3) >= 12 and lib.vfa_conv3x3_workspace_bytes(0) == 0
    assert lib.vfa_group_norm_workspace_bytes(2, 16) == 2 * 16 * 32 * 2 * 8 and lib.vfa_group_norm_workspace_bytes(2, 0) == 0
    stride = (ctypes.c_longlong * 4)(256 * 16, 16, 4, 1)
    negative = (ctypes.c_longlong * 4)(256 * 16, 16, -4, 1)
    p = ctypes.c_void_p(4096)   # (never dereferenced)
    nbytes = lib.vfa_conv3x3_packed_bytes(256, 256)

    def dense(B=1, C=256, L=4, W=4, O=256, d=1, x=p, stride=stride, packed=p, nbytes=nbytes, out=p, ws=p, ws_bytes=256):
        return lib.vfa_conv3x3_f32(x, stride, packed, nbytes, None, None, 0, B, C, L, W, O, d, out, ws, ws_bytes, None)

    def few(B=1, C=256, L=4, W=4, O=2, d=1, x=p, stride=stride, weight=p, a=None, b=None, out=p):
        return lib.vfa_conv3x3_few_f32(x, stride, weight, a, b, B, C, L, W, O, d, out, None)

    def gn(B=1, C=256, L=4, W=4, groups=16, x=p, stride=stride, a=p, b=p, ws=p, ws_bytes=1 << 20):
        return lib.vfa_group_norm_affine_f32(x, stride, None, None, 1e-5, B, C, L, W, groups, a, b, ws, ws_bytes, None)

    for call in (dense, few, gn):
        assert call(B=-1) == BAD and call(C=0) == BAD and call(L=-1) == BAD and call(W=-1) == BAD
        assert call(x=None) == BAD and call(stride=None) == BAD and call(stride=negative) == BAD
        assert call(B=70000) == UNSUPPORTED and call(L=1 << 15, W=1 << 15) == UNSUPPORTED
        assert call(B=0) == 0 and call(L=0) == 0 and call(W=0) == 0
    for call in (dense, few):
        assert call(O=0) == BAD and call(d=0) == BAD and call(d=5) == UNSUPPORTED and call(out=None) == BAD
    assert dense(C=48) == UNSUPPORTED and dense(packed=None) == BAD and dense(nbytes=nbytes - 1) == BAD
    assert dense(packed=ctypes.c_void_p(4100)) == BAD and dense(ws=None) == BAD and dense(ws_bytes=2) == BAD
    assert dense(O=360) == BAD                                       # (the packed planes were made for another O)
    assert few(O=5) == UNSUPPORTED and few(C=30) == UNSUPPORTED and few(weight=None) == BAD and few(a=p) == BAD and few(b=p) == BAD
    assert gn(groups=0) == BAD and gn(groups=7) == BAD and gn(a=None) == BAD and gn(ws=None) == BAD and gn(ws_bytes=8) == BAD
    assert gn(ws=ctypes.c_void_p(4100)) == BAD
    assert lib.vfa_conv3x3_pack_weights_f32(p, 256, 48, p, nbytes, None) == UNSUPPORTED
    assert lib.vfa_conv3x3_pack_weights_f32(None, 256, 256, p, nbytes, None) == BAD
    assert lib.vfa_conv3x3_pack_weights_f32(p, 256, 256, p, nbytes + 1, None) == BAD
    assert lib.vfa_bn_fold_f32(None, None, None, p, None, 1e-5, 4, p, p, None) == BAD
    assert lib.vfa_bn_fold_f32(None, None, p, p, None, 1e-5, 0, p, p, None) == 0


def _net(mode="3D"):
    from vfa_amd.vfanet import VFANet
    return VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base="resnet18", mode=mode)


def test_head_convs_attribute_and_argument():
    from vfa_amd import vfanet
    from vfa_amd.vfanet import VFANet
    assert vfanet.HEAD_CONVS == ("library", "hip")
    assert list(inspect.signature(VFANet.heads).parameters) == ["self", "topdown", "rotation_at", "convs"]
    assert inspect.signature(VFANet.heads).parameters["convs"].default is None
    net = _net().eval()
    assert net.head_convs == "library" and "head_convs" not in net.state_dict()
    topdown = torch.randn(1, 256, 6, 7)
    with torch.no_grad():
        want = net.heads(topdown)
        for bad in ("miopen", "", 1):
            with pytest.raises(ValueError, match="convs"):
                net.heads(topdown, convs=bad)
        net.head_convs = "nothing"
        with pytest.raises(ValueError, match="convs"):
            net.heads(topdown)
        assert sorted(net.heads(topdown, convs="library")) == sorted(want)   # the argument wins over the attribute
        # a CPU map is outside what "hip" covers: the library path, bit for bit
        net.head_convs = "hip"
        got = net.heads(topdown)
    assert sorted(got) == sorted(want) and all(torch.equal(got[k], want[k]) for k in want)


def test_state_dict_keys_do_not_change():
    a, b = _net("2D"), _net("2D")
    b.head_convs = "hip"
    assert list(a.state_dict()) == list(b.state_dict())


def test_wrappers_are_inference_only_and_refuse_cpu_tensors(built_lib):
    from vfa_amd import ops
    from vfa_amd._lib import VFAHipError
    assert list(inspect.signature(ops.conv3x3).parameters) == ["x", "weight", "dilation", "scale", "shift", "relu"]
    assert list(inspect.signature(ops.conv3x3_few).parameters) == ["x", "weight", "dilation", "affine"]
    assert list(inspect.signature(ops.group_norm_affine).parameters) == ["x", "groups", "weight", "bias", "eps"]
    x, w = torch.zeros(1, 32, 4, 4), torch.zeros(2, 32, 3, 3)
    for call in (lambda: ops.conv3x3(x, w), lambda: ops.conv3x3_few(x, w), lambda: ops.group_norm_affine(x, 4, None, None, 1e-5)):
        with pytest.raises(VFAHipError):
            call()
    xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
    for call in (lambda: ops.conv3x3(xg, w), lambda: ops.conv3x3(x, wg), lambda: ops.conv3x3_few(x, wg),
                 lambda: ops.group_norm_affine(xg, 4, None, None, 1e-5)):
        with pytest.raises(ValueError, match="inference only"):
            call()
    with torch.no_grad(), pytest.raises(VFAHipError):   # with gradients off a parameter is fine: only the device is refused
        ops.conv3x3(x, wg)
