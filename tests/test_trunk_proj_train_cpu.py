"""Training the trunk's projection blocks without a GPU: the header against ``_lib.SIGNATURES``; what the new entry points and
wrappers refuse before they launch; the workspaces as closed formulas; the ``trunk_proj_train`` attribute, which on CPU tensors leaves
``VFANet.trunk`` the library's in bits, gradients included; the float64 restatement of ``ops.projection_block_train``
(tests/trunk_proj_common.py) against float64 autograd of ``_Block(cin, cout, 2)``; and the integer rules of the two stride-2 gradients
(vfa_amd/csrc/vfa_conv_grad.h and the blocks of taps of vfa_conv.h, shared host / device code) compiled with g++ into
tests/native/trunk_down_harness.cpp and checked against brute force, once more as a stand-alone program under the host sanitizers."""
import ctypes
import inspect
import re
from types import SimpleNamespace

import pytest
import torch

import conv_common as cc
import trunk_proj_common as tp
import trunk_train_common as tt
from native_common import ABI_VERSION, build_harness, declared_parameters, run_harness

GXX_FLAGS = ["-O1", "-std=c++17", "-Wall"]
BAD, UNSUPPORTED = 10001, 10002
NEW_SYMBOLS = {"vfa_trunk_down_wgrad_workspace_bytes": 6, "vfa_trunk_down_wgrad_f32": 14, "vfa_trunk_down_dgrad_workspace_bytes": 4,
               "vfa_trunk_down_dgrad_f32": 16}


@pytest.fixture(scope="module")
def built_lib():
    from vfa_amd import build
    return build.build()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "trunk_down", "trunk_down_harness.cpp", GXX_FLAGS)


@pytest.fixture(scope="module")
def sanitized_harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "trunk_down", "trunk_down_harness.cpp", GXX_FLAGS, sanitized=True)


def test_rules_of_the_stride_2_gradients_against_brute_force(harness):
    positions, terms = (int(v) for v in re.findall(r"(\d+) (?:positions|terms)", run_harness(harness, "classes")))
    sizes = list(range(1, 10)) + [31, 32, 33, 64, 65, 66]
    assert positions == sum(sizes) ** 2 and 2 * positions < terms < 9 * positions // 4      # 9 tap products per 4 positions, less the borders
    pairs, indices = (int(v) for v in re.findall(r"(\d+) (?:pairs|indices)", run_harness(harness, "wgrad")))
    assert pairs > 500000 and indices == 2 * 3 * 64 * 32 * 10


def test_rules_of_the_stride_2_gradients_under_the_host_sanitizers(sanitized_harness):
    run_harness(sanitized_harness, "classes")
    run_harness(sanitized_harness, "wgrad")


def test_header_and_bindings_agree_on_the_new_symbols(built_lib):
    from vfa_amd import _lib
    declared = declared_parameters()
    lib = _lib.lib()
    for name, count in NEW_SYMBOLS.items():
        assert declared.get(name) == count == len(_lib.SIGNATURES[name]) and hasattr(lib, name), name
    assert _lib.ABI_VERSION == ABI_VERSION == 9 == lib.vfa_abi_version()


def test_workspaces_are_closed_formulas(built_lib):
    from vfa_amd import _lib
    lib = _lib.lib()
    ws = lib.vfa_trunk_down_wgrad_workspace_bytes                    # (B, O, C, L, W of x, kernel): pad256(8 B) + 4 B slabs_for kernel^2 O C
    assert ws(7, 128, 64, 180, 320, 3) == 256 + 7 * 16 * 9 * 128 * 64 * 4 and ws(7, 128, 64, 180, 320, 1) == 256 + 7 * 16 * 128 * 64 * 4
    assert ws(7, 512, 256, 45, 80, 3) == 256 + 7 * 6 * 9 * 512 * 256 * 4          # g is 23 x 40: 12 slabs, halved at 512 x 256
    assert ws(2, 128, 64, 9, 13, 3) == 256 + 2 * 2 * 9 * 128 * 64 * 4             # g is 5 x 7: two tiles
    assert ws(2, 128, 64, 1, 1, 1) == 256 + 2 * 128 * 64 * 4
    assert ws(0, 128, 64, 9, 13, 3) == 0 and ws(2, 128, 40, 9, 13, 3) == 0 and ws(2, 128, 64, 9, 13, 2) == 0 and ws(2, 128, 64, 0, 13, 3) == 0
    ws = lib.vfa_trunk_down_dgrad_workspace_bytes                    # (B, O, C, kernel): pad256(4 B) + 64 + 512 kernel^2 ceil(C / 128) O
    assert ws(7, 128, 64, 3) == 256 + 64 + 512 * 9 * 128 and ws(7, 512, 256, 1) == 256 + 64 + 512 * 2 * 512
    assert ws(100, 256, 128, 3) == 512 + 64 + 512 * 9 * 256
    assert ws(0, 128, 64, 3) == 0 and ws(2, 100, 64, 3) == 0 and ws(2, 128, 40, 3) == 0 and ws(2, 128, 64, 2) == 0


def test_refusals_of_the_entry_points(built_lib):
    """What the calls decide before they launch anything (no device is touched: every case returns first)."""
    from vfa_amd import _lib
    lib = _lib.lib()
    p, big = ctypes.c_void_p(4096), 1 << 30       # never dereferenced
    gs, xs = (ctypes.c_longlong * 4)(128 * 35, 35, 7, 1), (ctypes.c_longlong * 4)(64 * 117, 117, 13, 1)
    neg = (ctypes.c_longlong * 4)(64 * 117, 117, -13, 1)

    def wgrad(g=p, g_stride=gs, x=p, x_stride=xs, B=2, C=64, L=9, W=13, O=128, kernel=3, dw=p, ws=p, ws_bytes=big):
        return lib.vfa_trunk_down_wgrad_f32(g, g_stride, x, x_stride, B, C, L, W, O, kernel, dw, ws, ws_bytes, None)
    assert wgrad(g=None) == BAD and wgrad(x=None) == BAD and wgrad(g_stride=None) == BAD and wgrad(x_stride=None) == BAD and wgrad(dw=None) == BAD
    assert wgrad(kernel=2) == BAD and wgrad(kernel=0) == BAD and wgrad(kernel=9) == BAD and wgrad(B=-1) == BAD and wgrad(x_stride=neg) == BAD
    assert wgrad(C=48) == UNSUPPORTED and wgrad(O=100) == UNSUPPORTED and wgrad(B=70000, ws_bytes=1 << 50) == UNSUPPORTED
    need = lib.vfa_trunk_down_wgrad_workspace_bytes(2, 128, 64, 9, 13, 3)
    assert wgrad(ws=None) == BAD and wgrad(ws_bytes=need - 1) == BAD and wgrad(ws=ctypes.c_void_p(4104)) == BAD

    def dgrad(g=p, g_stride=gs, w=p, B=2, O=128, Lo=5, Wo=7, C=64, L=9, W=13, kernel=3, accumulate=0, dx=p, ws=p, ws_bytes=big):
        return lib.vfa_trunk_down_dgrad_f32(g, g_stride, w, B, O, Lo, Wo, C, L, W, kernel, accumulate, dx, ws, ws_bytes, None)
    assert dgrad(g=None) == BAD and dgrad(g_stride=None) == BAD and dgrad(w=None) == BAD and dgrad(dx=None) == BAD and dgrad(g_stride=neg) == BAD
    assert dgrad(kernel=2) == BAD and dgrad(accumulate=2) == BAD and dgrad(B=-1) == BAD
    assert dgrad(L=11) == BAD and dgrad(L=8) == BAD and dgrad(W=15) == BAD and dgrad(Lo=4) == BAD      # (L - 1) / 2 + 1 != Lo
    assert dgrad(C=48) == UNSUPPORTED and dgrad(O=100) == UNSUPPORTED and dgrad(kernel=1) == UNSUPPORTED
    need = lib.vfa_trunk_down_dgrad_workspace_bytes(2, 128, 64, 3)
    assert dgrad(ws=None) == BAD and dgrad(ws_bytes=need - 1) == BAD and dgrad(ws=ctypes.c_void_p(4104)) == BAD
    assert dgrad(B=0) == 0 and wgrad(ws_bytes=need - 1, C=48) == UNSUPPORTED


def test_wrappers_exist_and_reject_bad_shapes():
    from vfa_amd import ops
    from vfa_amd._lib import VFAHipError
    assert list(inspect.signature(ops.trunk_down_weight_grad).parameters) == ["grad", "x", "kernel"]
    assert list(inspect.signature(ops.trunk_down_input_grad).parameters)[:3] == ["grad", "weight", "size"]
    sig = inspect.signature(ops.projection_block_train)
    assert list(sig.parameters) == ["x", "w1", "g1", "b1", "w2", "g2", "b2", "wd", "gd", "bd", "groups", "eps"]
    assert sig.parameters["groups"].default == 16 and sig.parameters["eps"].default == 1e-5
    x, g = torch.zeros(2, 64, 9, 13), torch.zeros(2, 128, 5, 7)
    w1, w2, wd, ga = torch.zeros(128, 64, 3, 3), torch.zeros(128, 128, 3, 3), torch.zeros(128, 64, 1, 1), torch.ones(128)
    with pytest.raises(ValueError, match="kernel"):
        ops.trunk_down_weight_grad(g, x, 2)
    with pytest.raises(ValueError, match="stride-2"):
        ops.trunk_down_weight_grad(torch.zeros(2, 128, 5, 6), x, 3)
    with pytest.raises(ValueError, match="stride-2"):
        ops.trunk_down_weight_grad(g, torch.zeros(2, 64, 11, 13), 3)
    with pytest.raises(ValueError, match="multiples of 32"):
        ops.trunk_down_weight_grad(torch.zeros(2, 100, 5, 7), x, 3)
    with pytest.raises(ValueError, match="weight must be"):
        ops.trunk_down_input_grad(g, torch.zeros(128, 64, 2, 2), (9, 13))
    with pytest.raises(ValueError, match="multiples of 32"):
        ops.trunk_down_input_grad(g, torch.zeros(128, 40, 3, 3), (9, 13))
    with pytest.raises(ValueError, match="for size"):
        ops.trunk_down_input_grad(g, w1, (11, 13))                  # (11 - 1) // 2 + 1 is not 5
    with pytest.raises(ValueError, match="grad must be"):
        ops.trunk_down_input_grad(torch.zeros(2, 64, 5, 7), w1, (9, 13))
    with pytest.raises(ValueError, match="add_to"):
        ops.trunk_down_input_grad(g, wd, (9, 13))
    with pytest.raises(ValueError, match="add_to"):
        ops.trunk_down_input_grad(g, w1, (9, 13), add_to=torch.zeros(2, 64, 9, 12))
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.projection_block_train(torch.zeros(2, 40, 9, 13), w1, ga, ga, w2, ga, ga, wd, ga, ga)
    with pytest.raises(ValueError, match="a weight"):
        ops.projection_block_train(x, w1, ga, ga, w2, ga, ga, torch.zeros(128, 64, 3, 3), ga, ga)
    with pytest.raises(ValueError, match="a weight"):
        ops.projection_block_train(x, w1, ga, ga, torch.zeros(128, 64, 3, 3), ga, ga, wd, ga, ga)
    with pytest.raises(ValueError, match="GroupNorm parameter"):
        ops.projection_block_train(x, w1, ga, ga, w2, ga, ga, wd, ga, torch.ones(64))
    with pytest.raises(ValueError, match="groups"):
        ops.projection_block_train(x, w1, ga, ga, w2, ga, ga, wd, ga, ga, groups=24)
    for call in (lambda: ops.trunk_down_weight_grad(g, x, 3), lambda: ops.trunk_down_weight_grad(g, x, 1),
                 lambda: ops.trunk_down_input_grad(g, w1, (9, 13)), lambda: ops.trunk_down_input_grad(g, wd, (9, 13), add_to=x.clone()),
                 lambda: ops.projection_block_train(x, w1, ga, ga, w2, ga, ga, wd, ga, ga)):
        with pytest.raises(VFAHipError, match="CPU tensor"):      # well-formed operands: no fallback on the CPU
            call()


def _net():
    from vfa_amd.vfanet import VFANet
    return VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base="resnet18", mode="3D")


def test_trunk_proj_train_attribute():
    from vfa_amd import vfanet
    assert vfanet.TRUNK_PROJ_TRAIN == ("library", "hip") and vfanet.TRUNK_CONVS_TRAIN == ("library", "hip")
    torch.manual_seed(3)
    net, plain = _net().train(), _net().train()
    assert net.trunk_proj_train == "library" and net.trunk_convs_train == "library"
    net.trunk_proj_train = net.trunk_convs_train = "hip"
    assert list(net.state_dict()) == list(plain.state_dict())
    plain.load_state_dict(net.state_dict())
    blocks = [b for layer in (net.base.layer1, net.base.layer2, net.base.layer3, net.base.layer4) for b in layer]
    assert [b.is_projection for b in blocks] == [False, False, True, False, True, False, True, False]
    assert all(b.is_projection != b.is_identity for b in blocks)
    x = torch.randn(1, 3, 64, 96)       # CPU images: the condition does not hold, the library path runs
    cot = [torch.randn(1, c, 64 // s, 96 // s) for c, s in ((128, 8), (256, 16), (512, 32))]
    got, want = net.trunk(x), plain.base(x)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    torch.autograd.backward(got, cot)
    torch.autograd.backward(want, cot)
    for (k, p), (_, q) in zip(net.base.named_parameters(), plain.base.named_parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), k
    with torch.no_grad():
        assert all(torch.equal(g, w) for g, w in zip(net.trunk(x), plain.base(x)))
    net.trunk_proj_train = "fast"
    with pytest.raises(ValueError, match="trunk_proj_train"):
        net.trunk(x)


@pytest.mark.parametrize("pair, size", [((64, 128), (2, 12, 40)), ((64, 128), (1, 9, 13)), ((32, 64), (2, 1, 1)), ((32, 64), (1, 2, 3))])
def test_restated_projection_block_is_float64_autograd(pair, size):
    """The restatement the GPU tests take their float64 reference from: the node's steps, against autograd of the module."""
    B, L, W = size
    block = tp.block_of(*pair, seed=pair[0])
    x, g = tp.block_inputs(block, B, L, W, seed=pair[0] + 3)
    out, dx, grads = tp.block_restated(block, x, g)
    out64, dx64, grads64 = tt.block_step(block, x, g, torch.float64)
    assert sorted(grads) == sorted(grads64) == sorted(tp.PARAMS)
    assert torch.equal(out, out64)
    for what, a, b in [("dx", dx, dx64)] + [(k, grads[k], grads64[k]) for k in tp.PARAMS]:
        rel = cc.normwise(a.reshape(b.shape), b)
        print(f"{what}: {rel:.3g}")
        assert rel < 1e-12, what


@pytest.mark.parametrize("shape", tp.SHAPES)
def test_references_of_the_stride_2_gradients_are_the_defining_sums(shape):
    """``trunk_proj_common.grads`` against the sums of the header, written out: dW over the cells of g, dX over the taps that reach a
    position -- in integers, so that equality is exact."""
    B, C, O, L, W = shape
    C, O = 4, 3                                        # (the index rules do not depend on the widths)
    x, w, g = tp.integer_inputs(B, C, O, L, W, seed=L + W)
    dx64, dw64 = tp.grads(x, w, g, torch.float64)
    dw, dx = torch.zeros(O, C, 3, 3, dtype=torch.float64), torch.zeros(B, C, L, W, dtype=torch.float64)
    for i in range(tp.down(L)):
        for j in range(tp.down(W)):
            for ty in range(3):
                for tx in range(3):
                    y, xx = 2 * i + ty - 1, 2 * j + tx - 1
                    if 0 <= y < L and 0 <= xx < W:
                        dw[:, :, ty, tx] += torch.einsum("bo,bc->oc", g[:, :, i, j].double(), x[:, :, y, xx].double())
                        dx[:, :, y, xx] += g[:, :, i, j].double() @ w[:, :, ty, tx].double()
    assert torch.equal(dw, dw64) and torch.equal(dx, dx64)
