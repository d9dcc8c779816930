"""The trunk's stem without a GPU: the integer rules of vfa_amd/csrc/vfa_stem.h (shared host / device code) compiled with g++ into
tests/native/stem_harness.cpp and checked against brute force, once more as a stand-alone program under the host sanitizers; the
numpy restatement of the kernels' arithmetic (tests/stem_common.py) against the two yardsticks, with two wrong restatements failing
(E); the restated pooling against the float64 chain, with the wrong order failing; a restated ResNet-18 trunk against the float64
trunk; what the entry points refuse before they launch; the Python surface."""
import copy
import ctypes
import inspect
import re
from types import SimpleNamespace

import pytest
import torch

import conv_common as cc
import stem_common as sc
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
    return build_harness(tmp_path_factory, "stem", "stem_harness.cpp", GXX_FLAGS)


@pytest.fixture(scope="module")
def sanitized_harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "stem", "stem_harness.cpp", GXX_FLAGS, sanitized=True)


def test_output_sizes_tiles_windows_and_taps_against_the_enumeration(harness):
    out = run_harness(harness, "conv")
    cells, positions, outside, taps = (int(v) for v in re.findall(r"(\d+) (?:cells|positions|outside|taps)", out))
    assert cells > 100000 and positions > 1000000 and outside > 100000 and taps == 4 * 32 * 147


def test_packed_weight_index_is_a_bijection(harness):
    assert int(re.search(r"(\d+) weights", run_harness(harness, "weights")).group(1)) == 64 * 148


def test_pool_output_sizes_and_taps_against_the_enumeration(harness):
    assert int(re.search(r"(\d+) windows", run_harness(harness, "pool")).group(1)) > 20000


def test_integer_rules_under_the_host_sanitizers(sanitized_harness):
    for mode in ("conv", "weights", "pool"):
        run_harness(sanitized_harness, mode)


@pytest.mark.parametrize("O,L,W", [(64, 9, 11), (5, 19, 141), (64, 2, 3), (64, 1, 1)])
def test_restated_convolution_meets_both_yardsticks(O, L, W):
    x, w = sc.inputs(2, O, L, W, seed=O + L + W)
    y = sc.emulate_conv(x, w)
    assert tuple(y.shape) == (2, O, sc.out_size(L), sc.out_size(W))
    sc.check_both(y, x, w, f"restated O={O} {L}x{W}")
    assert torch.equal(y[1], sc.emulate_conv(x[1:], w)[0])            # per image: no scale, no statistic of the batch


def test_two_wrong_restatements_fail_the_elementwise_yardstick():
    """The yardstick discriminates before a GPU sees it: a window that starts one position off, and ky / kx exchanged on a weight
    that is not symmetric."""
    x, w = sc.inputs(2, 64, 9, 11, seed=7)
    assert not torch.equal(w, w.transpose(2, 3))
    sc.check_elementwise(sc.emulate_conv(x, w), x, w, "the kernel's order")
    with pytest.raises(AssertionError, match=r"\(E\)"):
        sc.check_elementwise(sc.emulate_conv(x, w, pad=2), x, w, "padding 2")
    with pytest.raises(AssertionError, match=r"\(E\)"):
        sc.check_elementwise(sc.emulate_conv(x, w, swap=True), x, w, "ky and kx exchanged")


@pytest.mark.parametrize("L,W", [(1, 1), (9, 11), (10, 70)])
def test_restated_pool_against_the_float64_chain_and_the_wrong_order_fails(L, W):
    gen = torch.Generator().manual_seed(L * W)
    y = torch.randn(2, 6, L, W, generator=gen) * 3
    affine = sc.pool_affine(2, 6, seed=L + W)
    assert float(affine[0].min()) < 0 < float(affine[0].max()) and float(affine[1].min()) < 0 < float(affine[1].max())
    if L > 1:
        y[1, 2, 4, 5] = float("nan")
    out = sc.emulate_pool(y, affine)
    assert tuple(out.shape) == (2, 6, sc.out_size(L), sc.out_size(W))
    sc.check_pool(out, y, affine, f"restated {L}x{W}")
    nan = torch.isnan(out)
    assert int(nan.sum()) == (0 if L == 1 else 2)                  # row 4 -> output row 2; column 5 -> outputs 2 and 3
    if L > 1:
        assert bool(nan[1, 2, 2, 2]) and bool(nan[1, 2, 2, 3])
        clean = y.nan_to_num(0.0)
        with pytest.raises(AssertionError, match="pool"):              # max before a negative a picks the wrong tap
            sc.check_pool(sc.emulate_pool(clean, affine, affine_last=True), clean, affine, "maximum first, affine after")
        positive = (affine[0].abs(), affine[1])
        sc.check_pool(sc.emulate_pool(clean, positive, affine_last=True), clean, positive, "maximum first with a > 0 (the orders agree)")


def _trunk(base="resnet18", seed=0):
    from vfa_amd.vfanet import _DEPTHS, _Trunk
    torch.manual_seed(seed)
    return tc.randomise_group_norms(_Trunk(_DEPTHS[base]), seed + 1).eval()


def test_restated_stem_and_trunk_against_the_float64_trunk():
    trunk = _trunk()
    x = torch.randn(2, 3, 64, 96, generator=torch.Generator().manual_seed(2))
    x[1] *= 1.7
    with torch.no_grad():
        lib32 = trunk(x)
        stem32 = trunk.stem(x)
        assert all(torch.equal(a, b) for a, b in zip(lib32, trunk.stages(stem32)))      # forward is stem + stages
        stem64 = copy.deepcopy(trunk).double().stem(x.double())
    cc.check_normwise(sc.emulate_stem(trunk, x), stem64, stem32, "restated stem")
    want64 = tc.module64(trunk, x)
    for name, y, y64, y32 in zip(("f8", "f16", "f32"), sc.emulate_trunk(trunk, x), want64, lib32):
        assert y.shape == y64.shape
        cc.check_normwise(y, y64, y32, f"restated trunk {name}")


def test_refusals_of_the_entry_points(built_lib):
    """What the calls decide before they launch anything (no device is touched: every case returns first)."""
    from vfa_amd import _lib
    lib = _lib.lib()
    assert lib.vfa_stem_workspace_bytes(64) == lib.vfa_stem_workspace_bytes(1) == 148 * 64 * 4
    assert lib.vfa_stem_workspace_bytes(0) == 0 and lib.vfa_stem_workspace_bytes(65) == 0 and lib.vfa_stem_workspace_bytes(-1) == 0
    stride = (ctypes.c_longlong * 4)(3 * 16, 16, 4, 1)
    negative = (ctypes.c_longlong * 4)(3 * 16, 16, -4, 1)
    huge = (ctypes.c_longlong * 4)(1 << 40, 1 << 31, 4, 1)
    p = ctypes.c_void_p(4096)   # (never dereferenced)
    ws_bytes = 148 * 64 * 4

    def conv(B=1, C=3, L=4, W=4, O=64, x=p, stride=stride, weight=p, out=p, ws=p, ws_bytes=ws_bytes):
        return lib.vfa_stem_conv_f32(x, stride, weight, B, C, L, W, O, out, ws, ws_bytes, None)

    def pool(B=1, C=64, L=4, W=4, y=p, a=p, b=p, out=p):
        return lib.vfa_stem_pool_f32(y, a, b, B, C, L, W, out, None)

    for call in (conv, pool):
        assert call(B=-1) == BAD and call(L=-1) == BAD and call(W=-1) == BAD and call(out=None) == BAD
        assert call(B=70000) == UNSUPPORTED and call(L=70000) == UNSUPPORTED and call(L=1 << 15, W=1 << 15) == UNSUPPORTED
        assert call(B=0) == 0 and call(L=0) == 0 and call(W=0) == 0
    assert conv(C=0) == BAD and conv(O=0) == BAD and conv(x=None) == BAD and conv(stride=None) == BAD and conv(stride=negative) == BAD
    assert conv(weight=None) == BAD and conv(ws=None) == BAD and conv(ws_bytes=ws_bytes - 1) == BAD and conv(ws=ctypes.c_void_p(4100)) == BAD
    assert conv(C=4) == UNSUPPORTED and conv(C=32) == UNSUPPORTED and conv(O=65) == UNSUPPORTED and conv(stride=huge) == UNSUPPORTED
    assert pool(C=-1) == BAD and pool(C=0) == 0 and pool(y=None) == BAD and pool(a=None) == BAD and pool(b=None) == BAD
    assert pool(B=65535, C=65535) == UNSUPPORTED


def _net(base="resnet18", mode="2D"):
    from vfa_amd.vfanet import VFANet
    return VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base=base, mode=mode)


def test_trunk_stem_attribute():
    from vfa_amd import vfanet
    assert vfanet.TRUNK_STEM == ("library", "hip") and vfanet.TRUNK_CONVS == ("library", "hip")
    net = _net().eval()
    assert net.trunk_stem == "library" and net.trunk_convs == "library" and "trunk_stem" not in net.state_dict()
    x = torch.randn(1, 3, 32, 32)
    with torch.no_grad():
        want = net.base(x)
        assert all(torch.equal(g, w) for g, w in zip(net.trunk(x), want))
        for bad in ("miopen", "", 1, None):
            net.trunk_stem = bad
            with pytest.raises(ValueError, match="trunk_stem"):
                net.trunk(x)
            with pytest.raises(ValueError, match="trunk_stem"):
                net.laterals(x)
        net.trunk_stem, net.trunk_convs = "hip", "nothing"
        with pytest.raises(ValueError, match="trunk_convs"):          # each bad value is named by its own attribute
            net.trunk(x)
        # a CPU tensor is outside what "hip" covers: the library path, bit for bit, with the other setting on either side
        for convs in ("library", "hip"):
            net.trunk_stem, net.trunk_convs = "hip", convs
            got = net.trunk(x)
            lats = net.laterals(x)
            assert len(got) == 3 and all(torch.equal(g, w) for g, w in zip(got, want))
            net.trunk_stem = net.trunk_convs = "library"
            assert all(torch.equal(g, w) for g, w in zip(lats, net.laterals(x)))


def test_state_dict_keys_do_not_change():
    for base in ("resnet18", "resnet34"):
        a, b = _net(base), _net(base)
        b.trunk_stem = "hip"
        assert list(a.state_dict()) == list(b.state_dict())
        assert [n for n, _ in a.named_modules()] == [n for n, _ in b.named_modules()]


def test_wrappers_are_inference_only_and_refuse_cpu_tensors(built_lib):
    from vfa_amd import ops
    from vfa_amd._lib import VFAHipError
    assert list(inspect.signature(ops.stem_conv).parameters) == ["x", "weight"]
    assert list(inspect.signature(ops.stem_pool).parameters) == ["y", "affine"]
    x, w = torch.zeros(1, 3, 8, 8), torch.zeros(64, 3, 7, 7)
    y, ab = torch.zeros(1, 64, 4, 4), (torch.ones(1, 64), torch.zeros(1, 64))
    for call in (lambda: ops.stem_conv(x, w), lambda: ops.stem_pool(y, ab)):
        with pytest.raises(VFAHipError):
            call()
    xg, wg, yg, ag = x.clone().requires_grad_(), w.clone().requires_grad_(), y.clone().requires_grad_(), ab[0].clone().requires_grad_()
    for call in (lambda: ops.stem_conv(xg, w), lambda: ops.stem_conv(x, wg), lambda: ops.stem_pool(yg, ab), lambda: ops.stem_pool(y, (ag, ab[1]))):
        with pytest.raises(ValueError, match="inference only"):
            call()
    with torch.no_grad(), pytest.raises(VFAHipError):   # with gradients off a parameter is fine: only the device is refused
        ops.stem_conv(x, wg)
