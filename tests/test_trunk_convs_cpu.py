"""The trunk's convolutions without a GPU: the integer rules of vfa_amd/csrc/vfa_conv.h (shared host / device code) compiled with g++
into tests/native/trunk_harness.cpp and checked against brute force, once more as a stand-alone program under the host sanitizers;
the numpy restatement of the kernels' arithmetic (tests/trunk_common.py) against the two yardsticks, with the restatement that drops
the lo pieces failing (N); a restated ResNet-18 trunk against the float64 trunk; what the entry points refuse before they launch; the
Python surface."""
import ctypes
import inspect
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import conv_common as cc
import trunk_common as tc
from native_common import build_harness, run_harness

GXX_FLAGS = ["-O1", "-std=c++17", "-Wall"]
BAD, UNSUPPORTED = 10001, 10002


@pytest.fixture(scope="module")
def built_lib():
    from vfa_amd import build
    return build.build()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "trunk", "trunk_harness.cpp", GXX_FLAGS)


@pytest.fixture(scope="module")
def sanitized_harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "trunk", "trunk_harness.cpp", GXX_FLAGS, sanitized=True)


def test_output_sizes_tiles_windows_and_taps_against_the_enumeration(harness):
    out = run_harness(harness, "tiles")
    cells, taps, outside, locations = (int(v) for v in re.findall(r"(\d+) (?:cells|taps|outside|locations)", out))
    assert cells > 100000 and taps > 1000000 and outside > 100000 and locations > 100000


def test_packed_weight_index_with_one_and_nine_taps_is_a_bijection(harness):
    out = run_harness(harness, "weights")
    assert int(re.search(r"(\d+) weights", out).group(1)) > 1000000


def test_integer_rules_under_the_host_sanitizers(sanitized_harness):
    run_harness(sanitized_harness, "tiles")
    run_harness(sanitized_harness, "weights")


@pytest.mark.parametrize("C,O,L,W,k,stride,prologue", [(64, 5, 9, 11, 3, 2, True), (128, 4, 9, 11, 1, 2, False), (512, 3, 6, 7, 3, 1, False)])
def test_restated_arithmetic_meets_both_yardsticks_and_dropping_lo_fails(C, O, L, W, k, stride, prologue):
    """C = 512 in the form the kernel uses: two chains of 256 channels, added once."""
    x, w = tc.inputs(2, C, O, L, W, seed=C + stride, k=k, nonneg=not prologue)
    affine = tc.affine_of(2, C, seed=C) if prologue else None
    y = tc.emulate_conv(x, w, stride, affine)
    assert tuple(y.shape) == (2, O, tc.out_size(L, stride), tc.out_size(W, stride))
    tc.check_both(y, x, w, stride, affine, f"restated C={C} k={k} stride={stride}")
    coarse = tc.emulate_conv(x, w, stride, affine, drop_lo=True)
    y64 = tc.conv(tc.prologue(x, affine, torch.float64), w, stride, torch.float64)
    y32 = tc.conv(tc.prologue(x, affine, torch.float32), w, stride, torch.float32)
    assert cc.normwise(coarse, y64) > 1e-4                      # an fp16 product: three orders of magnitude off
    with pytest.raises(AssertionError, match=r"\(N\)"):
        cc.check_normwise(coarse, y64, y32, "hi pieces alone")


def test_restatement_is_the_heads_restatement_at_stride_one_and_per_image():
    x, w = tc.inputs(2, 64, 3, 5, 6, seed=3)
    assert torch.equal(tc.emulate_conv(x, w, 1), cc.emulate_dense(x, w, 1))
    x[1] *= 1000.0
    affine = tc.affine_of(2, 64, seed=4)
    assert torch.equal(tc.emulate_conv(x, w, 2, affine)[0], tc.emulate_conv(x[:1], w, 2, (affine[0][:1], affine[1][:1]))[0])


def test_restated_scale_sees_what_the_products_see():
    """A huge value that the prologue clamps, or that a strided 1 x 1 convolution never reads, must not set the image's scale."""
    x, w = tc.inputs(1, 32, 2, 6, 6, seed=5, k=1)
    big = x.clone()
    big[0, 0, 1, 1] = 1e30                                      # an odd position: not read at stride 2
    with np.errstate(over="ignore"):                           # (the restatement splits the whole map, the unread value included)
        assert torch.equal(tc.emulate_conv(x, w, 2), tc.emulate_conv(big, w, 2))
    x3, w3 = tc.inputs(1, 32, 2, 6, 6, seed=6)
    affine = (torch.ones(1, 32), torch.zeros(1, 32))
    low = x3.clone()
    low[0, 0, 2, 2] = -1e30                                     # relu(-1e30) = 0
    zeroed = x3.clone()
    zeroed[0, 0, 2, 2] = -1.0
    assert torch.equal(tc.emulate_conv(low, w3, 1, affine), tc.emulate_conv(zeroed, w3, 1, affine))


def _trunk(base="resnet18", seed=0):
    from vfa_amd.vfanet import _DEPTHS, _Trunk
    torch.manual_seed(seed)
    return tc.randomise_group_norms(_Trunk(_DEPTHS[base]), seed + 1).eval()


def test_restated_resnet18_trunk_against_the_float64_trunk():
    trunk = _trunk()
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(2))
    x[1] *= 1.7
    with torch.no_grad():
        lib32 = trunk(x)
    want64 = tc.module64(trunk, x)
    got = tc.emulate_trunk(trunk, x)
    for name, y, y64, y32 in zip(("f8", "f16", "f32"), got, want64, lib32):
        assert y.shape == y64.shape
        cc.check_normwise(y, y64, y32, f"restated trunk {name}")


def test_restated_block_join_keeps_a_nan_to_its_element():
    y = torch.randn(1, 2, 3, 4)
    y[0, 1, 2, 3] = float("nan")
    out = tc.emulate_join(y, (torch.ones(1, 2), torch.zeros(1, 2)), torch.randn(1, 2, 3, 4))
    nan = torch.isnan(out)
    assert int(nan.sum()) == 1 and bool(nan[0, 1, 2, 3]) and float(out[~nan].min()) >= 0.0


def test_refusals_of_the_entry_points(built_lib):
    """What the calls decide before they launch anything (no device is touched: every case returns first)."""
    from vfa_amd import _lib
    lib = _lib.lib()
    assert lib.vfa_trunk_packed_bytes(256, 256, 9) == lib.vfa_conv3x3_packed_bytes(256, 256) == 64 + 256 * 256 * 9 * 2 * 2
    assert lib.vfa_trunk_packed_bytes(1, 32, 1) == 64 + 128 * 32 * 2 * 2              # outputs are padded to the tile, one tap per chunk
    assert lib.vfa_trunk_packed_bytes(256, 48, 9) == 0 and lib.vfa_trunk_packed_bytes(0, 32, 9) == 0
    assert lib.vfa_trunk_packed_bytes(256, 64, 3) == 0 and lib.vfa_trunk_packed_bytes(256, 64, 0) == 0
    assert lib.vfa_trunk_workspace_bytes(3) >= 12 and lib.vfa_trunk_workspace_bytes(0) == 0 and lib.vfa_trunk_workspace_bytes(-1) == 0
    stride = (ctypes.c_longlong * 4)(64 * 16, 16, 4, 1)
    negative = (ctypes.c_longlong * 4)(64 * 16, 16, -4, 1)
    p = ctypes.c_void_p(4096)   # (never dereferenced)
    nbytes = lib.vfa_trunk_packed_bytes(128, 64, 9)

    def conv(B=1, C=64, L=4, W=4, O=128, taps=9, s=2, x=p, stride=stride, packed=p, nbytes=nbytes, a=None, b=None, out=p, ws=p, ws_bytes=256):
        return lib.vfa_trunk_conv_f32(x, stride, packed, nbytes, a, b, B, C, L, W, O, taps, s, out, ws, ws_bytes, None)

    def join(B=1, C=64, L=4, W=4, y=p, a=p, b=p, r=p, ra=None, rb=None, out=p):
        return lib.vfa_residual_join_f32(y, a, b, r, ra, rb, B, C, L, W, out, None)

    for call in (conv, join):
        assert call(B=-1) == BAD and call(L=-1) == BAD and call(W=-1) == BAD and call(out=None) == BAD
        assert call(B=70000) == UNSUPPORTED and call(L=70000) == UNSUPPORTED and call(L=1 << 15, W=1 << 15) == UNSUPPORTED
        assert call(B=0) == 0 and call(L=0) == 0 and call(W=0) == 0
    assert conv(C=0) == BAD and conv(O=0) == BAD and conv(x=None) == BAD and conv(stride=None) == BAD and conv(stride=negative) == BAD
    assert conv(taps=3) == BAD and conv(taps=0) == BAD and conv(s=0) == BAD and conv(s=3) == BAD
    assert conv(a=p) == BAD and conv(b=p) == BAD
    assert conv(C=48) == UNSUPPORTED and conv(packed=None) == BAD and conv(nbytes=nbytes - 1) == BAD
    assert conv(packed=ctypes.c_void_p(4100)) == BAD and conv(ws=None) == BAD and conv(ws_bytes=2) == BAD
    assert conv(taps=1) == BAD and conv(O=360) == BAD                # (the packed planes were made for other taps, another O)
    assert join(C=-1) == BAD and join(C=0) == 0 and join(y=None) == BAD and join(a=None) == BAD and join(b=None) == BAD and join(r=None) == BAD
    assert join(ra=p) == BAD and join(rb=p) == BAD
    assert lib.vfa_trunk_pack_weights_f32(p, 256, 48, 9, p, nbytes, None) == UNSUPPORTED
    assert lib.vfa_trunk_pack_weights_f32(None, 128, 64, 9, p, nbytes, None) == BAD
    assert lib.vfa_trunk_pack_weights_f32(p, 128, 64, 3, p, nbytes, None) == BAD
    assert lib.vfa_trunk_pack_weights_f32(p, 128, 64, 9, p, nbytes + 1, None) == BAD
    assert lib.vfa_trunk_pack_weights_f32(p, 128, 64, 9, ctypes.c_void_p(4100), nbytes, None) == BAD


def _net(base="resnet18", mode="2D"):
    from vfa_amd.vfanet import VFANet
    return VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base=base, mode=mode)


def test_trunk_convs_attribute():
    from vfa_amd import vfanet
    from vfa_amd.vfanet import VFANet
    assert vfanet.TRUNK_CONVS == ("library", "hip")
    assert list(inspect.signature(VFANet.trunk).parameters) == ["self", "x"]
    net = _net().eval()
    assert net.trunk_convs == "library" and "trunk_convs" not in net.state_dict()
    x = torch.randn(1, 3, 32, 32)
    with torch.no_grad():
        want = net.base(x)
        got = net.trunk(x)
        assert all(torch.equal(g, w) for g, w in zip(got, want))
        for bad in ("miopen", "", 1, None):
            net.trunk_convs = bad
            with pytest.raises(ValueError, match="trunk_convs"):
                net.trunk(x)
            with pytest.raises(ValueError, match="trunk_convs"):
                net.laterals(x)
        # a CPU tensor is outside what "hip" covers: the library path, bit for bit
        net.trunk_convs = "hip"
        got = net.trunk(x)
        lats = net.laterals(x)
        net.trunk_convs = "library"
        lats_lib = net.laterals(x)
    assert len(got) == 3 and all(torch.equal(g, w) for g, w in zip(got, want))
    assert all(torch.equal(g, w) for g, w in zip(lats, lats_lib))


def test_laterals_and_lateral_integrals_go_through_trunk():
    """One method in front of the trunk: both producers call it (a replaced ``trunk`` is what they read, and ``base`` is not called
    beside it).  ``lateral_integrals`` has no CPU form behind the trunk, so its two branches are stopped at the replaced method."""
    class Reached(Exception):
        pass

    net = _net().eval()
    seen = []
    real = net.trunk
    net.trunk = lambda x: (seen.append(tuple(x.shape)), real(x))[1]
    x = torch.randn(1, 3, 32, 32)
    with torch.no_grad():
        net.laterals(x)
    assert seen == [(1, 3, 32, 32)]

    def stop(x):
        seen.append(tuple(x.shape))
        raise Reached
    net.trunk = stop
    net.base.forward = lambda x: pytest.fail("the trunk was called around VFANet.trunk")
    with pytest.raises(Reached):                                     # gradients enabled: the training branch
        net.lateral_integrals(x)
    with torch.no_grad(), pytest.raises(Reached):
        net.lateral_integrals(x)
    with torch.no_grad(), pytest.raises(Reached):
        net.laterals(x)
    assert seen == [(1, 3, 32, 32)] * 4


def test_state_dict_keys_do_not_change():
    for base in ("resnet18", "resnet34"):
        a, b = _net(base), _net(base)
        b.trunk_convs = "hip"
        assert list(a.state_dict()) == list(b.state_dict())


def test_wrappers_are_inference_only_and_refuse_cpu_tensors(built_lib):
    from vfa_amd import ops
    from vfa_amd._lib import VFAHipError
    assert list(inspect.signature(ops.trunk_conv).parameters) == ["x", "weight", "stride", "affine"]
    assert list(inspect.signature(ops.residual_join).parameters)[:4] == ["y", "affine", "shortcut", "shortcut_affine"]
    assert ops._CONV_KEPT_MAX >= 36 + 10                              # a ResNet-34 trunk beside the heads' entries
    x, w, w1 = torch.zeros(1, 32, 4, 4), torch.zeros(2, 32, 3, 3), torch.zeros(2, 32, 1, 1)
    ab = (torch.ones(1, 32), torch.zeros(1, 32))
    for call in (lambda: ops.trunk_conv(x, w), lambda: ops.trunk_conv(x, w1, 2), lambda: ops.residual_join(x, ab, x)):
        with pytest.raises(VFAHipError):
            call()
    xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
    for call in (lambda: ops.trunk_conv(xg, w), lambda: ops.trunk_conv(x, wg), lambda: ops.residual_join(xg, ab, x),
                 lambda: ops.residual_join(x, ab, xg)):
        with pytest.raises(ValueError, match="inference only"):
            call()
    with torch.no_grad(), pytest.raises(VFAHipError):   # with gradients off a parameter is fine: only the device is refused
        ops.trunk_conv(x, wg)
