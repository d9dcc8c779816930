"""The gradients of the dense 3x3 convolution without a GPU: the numpy restatement of the weight-gradient kernel's arithmetic
(tests/conv_grad_common.py) against the two yardsticks on the shapes of the GPU tests, with three wrong restatements that must fail
them; the transposed, tap-mirrored weight identity of the input gradient, exactly; the slab rule of vfa_amd/csrc/vfa_conv_grad.h
(shared host / device code) compiled with g++ into tests/native/conv_grad_harness.cpp and checked against brute force, once more as
a stand-alone program under the host sanitizers; the header against ``_lib.SIGNATURES``; what the entry points refuse before they
launch; the Python surface."""
import ctypes
import inspect
import re
from types import SimpleNamespace

import pytest
import torch

import conv_common as cc
import conv_grad_common as cg
from native_common import ABI_VERSION, build_harness, declared_parameters, run_harness

GXX_FLAGS = ["-O1", "-std=c++17", "-Wall"]
BAD, UNSUPPORTED = 10001, 10002
NEW_SYMBOLS = {"vfa_conv3x3_pack_weights_transposed_f32": 6, "vfa_conv3x3_wgrad_workspace_bytes": 5, "vfa_conv3x3_wgrad_f32": 15}
SHAPES = {  # name: (B, C, O, L, W, dilation): the shapes of tests/test_conv_grad.py
    "A": (2, 64, 96, 9, 37, 1),
    "B": (2, 32, 32, 3, 5, 4),
    "C_d1": (2, 256, 256, 20, 24, 1),
    "C_d2": (2, 256, 256, 20, 24, 2),
}


@pytest.fixture(scope="module")
def built_lib():
    from vfa_amd import build
    return build.build()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "conv_grad", "conv_grad_harness.cpp", GXX_FLAGS)


@pytest.fixture(scope="module")
def sanitized_harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "conv_grad", "conv_grad_harness.cpp", GXX_FLAGS, sanitized=True)


def test_slab_rule_covers_every_cell_once(harness):
    out = run_harness(harness, "slabs")
    cells, slabs = (int(v) for v in re.findall(r"(\d+) (?:cells|slabs)", out))
    assert cells >= sum(L * W for L in range(1, 71) for W in range(1, 71)) and slabs > 4900
    out = run_harness(harness, "partials")
    assert int(re.search(r"(\d+) indices", out).group(1)) > 100000


def test_slab_rule_under_the_host_sanitizers(sanitized_harness):
    run_harness(sanitized_harness, "slabs")
    run_harness(sanitized_harness, "partials")


def test_restated_slab_rule_is_the_headers():
    """The Python restatement the emulation uses, on the sizes the tests and the benchmark use."""
    assert [cg.slabs(L, W) for L, W in ((3, 5), (9, 37), (20, 24), (156, 156), (200, 200))] == [1, 6, 5, 16, 16]
    for L, W in ((9, 37), (20, 24), (37, 70), (156, 156)):
        seen = [t for s in range(cg.slabs(L, W)) for t in cg.slab_tiles(s, L, W)]
        assert seen == list(range(cg.tiles(L, W))) and all(len(cg.slab_tiles(s, L, W)) for s in range(cg.slabs(L, W)))


@pytest.mark.parametrize("name", list(SHAPES))
def test_restated_weight_gradient_meets_both_yardsticks(name):
    B, C, O, L, W, d = SHAPES[name]
    x, _, g = cg.inputs(B, C, O, L, W, seed=C + d)
    dw = cg.emulate_wgrad(g, x, d)
    cg.check_elementwise(dw, g, x, d, f"restated wgrad {name}")
    cg.check_normwise(dw, cg.wgrad64(g, x, d), cg.wgrad32(g, x, d), f"restated wgrad {name}")


@pytest.mark.parametrize("variant", ["hi", "mirror", "edge"])
def test_wrong_restatements_fail_a_yardstick(variant):
    """The hi pieces alone, a mirrored tap and edge padding in place of zeros: each must fail (E) or (N) on shape A."""
    B, C, O, L, W, d = SHAPES["A"]
    x, _, g = cg.inputs(B, C, O, L, W, seed=C + d)
    dw = cg.emulate_wgrad(g, x, d, variant=variant)
    with pytest.raises(AssertionError, match=r"\((E|N)\)"):
        cg.check_elementwise(dw, g, x, d, variant)
        cg.check_normwise(dw, cg.wgrad64(g, x, d), cg.wgrad32(g, x, d), variant)


def test_restated_weight_gradient_is_a_merge_of_per_frame_partials():
    """A frame's partials come from that frame alone: the bits of a frame alone and in a batch whose other frame is 1000 times
    larger; the batch is the documented merge."""
    B, C, O, L, W, d = 2, 32, 32, 9, 37, 2
    x, _, g = cg.inputs(B, C, O, L, W, seed=5)
    x[1] *= 1000.0
    both = cg.emulate_wgrad(g, x, d, per_frame=True)
    assert both.shape == (B, cg.slabs(L, W), O, C, 3, 3)
    for b in range(B):
        assert torch.equal(both[b], cg.emulate_wgrad(g[b:b + 1], x[b:b + 1], d, per_frame=True)[0])
    assert torch.equal(cg.merge_partials(both), cg.emulate_wgrad(g, x, d))


@pytest.mark.parametrize("d", [1, 2, 4])
def test_input_gradient_is_the_convolution_with_the_transposed_flipped_weight(d):
    """Exactly, in float64 on integer-valued inputs: conv64(g, w', d) == autograd's dX with w'[c, o, ty, tx] = w[o, c, 2 - ty, 2 - tx]."""
    gen = torch.Generator().manual_seed(d)
    B, C, O, L, W = 2, 5, 7, 6, 9
    x = torch.randint(-8, 9, (B, C, L, W), generator=gen).double()
    w = torch.randint(-8, 9, (O, C, 3, 3), generator=gen).double()
    g = torch.randint(-8, 9, (B, O, L, W), generator=gen).double()
    dx = cg.grads64(x, w, g, d)[0]
    assert torch.equal(cc.conv64(g, cg.transposed_flipped(w), d), dx) and dx.abs().max() > 0


def test_header_and_bindings_agree_on_the_new_symbols(built_lib):
    from vfa_amd import _lib
    declared = declared_parameters()
    lib = _lib.lib()
    for name, count in NEW_SYMBOLS.items():
        assert declared.get(name) == count == len(_lib.SIGNATURES[name]) and hasattr(lib, name), name
    assert _lib.ABI_VERSION == ABI_VERSION == 9 == lib.vfa_abi_version()
    makefile = open(built_lib.replace("libvfa_hip.so", "Makefile")).read()
    assert "vfa_conv_grad.hip" in makefile.split("SRCS")[1] and "vfa_conv_grad.h" in makefile.split("HDRS")[1]


def test_refusals_of_the_entry_points(built_lib):
    """What the calls decide before they launch anything (no device is touched: every case returns first)."""
    from vfa_amd import _lib
    lib = _lib.lib()
    per = 9 * 256 * 256 * 4
    assert lib.vfa_conv3x3_wgrad_workspace_bytes(1, 256, 256, 3, 5) == 256 + per
    assert lib.vfa_conv3x3_wgrad_workspace_bytes(4, 256, 256, 156, 156) == 256 + 4 * 16 * per
    assert lib.vfa_conv3x3_wgrad_workspace_bytes(2, 96, 64, 9, 37) == 256 + 2 * 6 * 9 * 96 * 64 * 4
    for sizes in ((0, 32, 32, 3, 5), (1, 40, 32, 3, 5), (1, 32, 48, 3, 5), (1, 32, 32, 0, 5), (70000, 32, 32, 3, 5)):
        assert lib.vfa_conv3x3_wgrad_workspace_bytes(*sizes) == 0, sizes
    stride = (ctypes.c_longlong * 4)(480, 15, 5, 1)
    p = ctypes.c_void_p(4096)   # never dereferenced: every case below returns before a launch
    wgrad = lib.vfa_conv3x3_wgrad_f32
    assert wgrad(p, stride, p, stride, 1, 32, 3, 5, 32, 1, None, None, p, 1 << 30, None) == BAD         # no dw
    assert wgrad(p, stride, p, stride, 1, 32, 3, 5, 32, 0, p, None, p, 1 << 30, None) == BAD            # dilation 0
    assert wgrad(p, stride, p, stride, 1, 32, 3, 5, 32, 5, p, None, p, 1 << 30, None) == UNSUPPORTED    # dilation 5
    assert wgrad(p, stride, p, stride, 1, 48, 3, 5, 32, 1, p, None, p, 1 << 30, None) == UNSUPPORTED    # C % 32
    assert wgrad(p, stride, p, stride, 1, 32, 3, 5, 40, 1, p, None, p, 1 << 30, None) == UNSUPPORTED    # O % 32
    assert wgrad(None, stride, p, stride, 1, 32, 3, 5, 32, 1, p, None, p, 1 << 30, None) == BAD         # no g
    assert wgrad(p, stride, p, None, 1, 32, 3, 5, 32, 1, p, None, p, 1 << 30, None) == BAD              # no strides
    assert wgrad(p, (ctypes.c_longlong * 4)(480, -15, 5, 1), p, stride, 1, 32, 3, 5, 32, 1, p, None, p, 1 << 30, None) == BAD
    assert wgrad(p, stride, p, stride, 1, 32, 3, 5, 32, 1, p, None, p, 255, None) == BAD                # a short workspace
    assert wgrad(p, stride, p, stride, 1, 32, 3, 5, 32, 1, p, None, ctypes.c_void_p(4100), 1 << 30, None) == BAD   # misaligned
    pack_t = lib.vfa_conv3x3_pack_weights_transposed_f32
    nbytes = lib.vfa_conv3x3_packed_bytes(64, 96)   # the planes of a convolution with 96 inputs and 64 outputs
    assert pack_t(p, 96, 64, p, nbytes + 2, None) == BAD
    assert pack_t(None, 96, 64, p, nbytes, None) == BAD
    assert pack_t(p, 40, 64, p, nbytes, None) == UNSUPPORTED   # O % 32: the inputs of the transposed convolution


def _net(mode="3D"):
    from vfa_amd.vfanet import VFANet
    return VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base="resnet18", mode=mode)


def test_head_convs_train_attribute():
    from vfa_amd import vfanet
    assert vfanet.HEAD_CONVS_TRAIN == ("library", "hip")
    net, plain = _net(), _net()
    assert net.head_convs_train == "library" and net.head_convs == "library"
    net.head_convs_train = "hip"
    assert list(net.state_dict()) == list(plain.state_dict())
    plain.load_state_dict(net.state_dict())
    topdown = torch.randn(1, 256, 5, 7, requires_grad=True)   # a CPU map: the condition does not hold, the library path runs
    got, want = net.heads(topdown), plain.heads(topdown)
    assert sorted(got) == sorted(want) and all(torch.equal(got[k], want[k]) for k in want)
    net.head_convs_train = "fast"
    with pytest.raises(ValueError, match="head_convs_train"):
        net.heads(topdown)


def test_train_wrapper_validates_like_the_inference_wrappers(built_lib):
    from vfa_amd import ops
    from vfa_amd._lib import VFAHipError
    assert list(inspect.signature(ops.conv3x3_train).parameters) == ["x", "weight", "bias", "dilation"]
    x, w = torch.zeros(1, 32, 3, 5, requires_grad=True), torch.zeros(32, 32, 3, 3, requires_grad=True)
    with pytest.raises(VFAHipError, match="CPU tensor"):   # (and not "inference only": operands that require grad are its business)
        ops.conv3x3_train(x, w)
