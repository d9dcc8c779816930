"""Training the trunk's identity residual blocks without a GPU: the header against ``_lib.SIGNATURES``; what the new entry points and
wrappers refuse before they launch; the ``trunk_convs_train`` attribute, which on CPU tensors leaves ``VFANet.trunk`` the library's
in bits, gradients included; the float64 restatement of the three-launch GroupNorm backward (tests/trunk_train_common.py) against
float64 autograd; the (E) yardstick of that backward, which accepts the restatement as the kernel rounds it and rejects two wrong
ones; and the slab rule of the trunk's weight gradient (``slabs_for`` of vfa_amd/csrc/vfa_conv_grad.h, shared host / device code)
compiled with g++ into tests/native/trunk_grad_harness.cpp and checked against brute force, once more as a stand-alone program under
the host sanitizers."""
import ctypes
import inspect
import re
from types import SimpleNamespace

import pytest
import torch

import conv_common as cc
import trunk_train_common as tt
from native_common import ABI_VERSION, build_harness, declared_parameters, run_harness

GXX_FLAGS = ["-O1", "-std=c++17", "-Wall"]
BAD, UNSUPPORTED = 10001, 10002
NEW_SYMBOLS = {"vfa_group_norm_stats_f32": 16, "vfa_group_norm_backward_workspace_bytes": 2, "vfa_group_norm_backward_f32": 20,
               "vfa_trunk_conv_wgrad_workspace_bytes": 5, "vfa_trunk_conv_wgrad_f32": 15}
GN_SHAPES = [(2, 64, 9, 13), (1, 512, 3, 5), (2, 128, 8, 32)]   # the shapes of tests/test_trunk_train.py
GROUPS, EPS = 16, 1e-5


@pytest.fixture(scope="module")
def built_lib():
    from vfa_amd import build
    return build.build()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "trunk_grad", "trunk_grad_harness.cpp", GXX_FLAGS)


@pytest.fixture(scope="module")
def sanitized_harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "trunk_grad", "trunk_grad_harness.cpp", GXX_FLAGS, sanitized=True)


def test_slab_rule_of_the_trunk_covers_every_cell_once(harness):
    out = run_harness(harness, "slabs")
    cells, rules, fewer = (int(v) for v in re.findall(r"(\d+) (?:cells|rules|fewer)", out))
    assert cells > 1000000 and rules >= 25 * (48 * 48 + 6) and fewer > 1000
    assert int(re.search(r"(\d+) indices", run_harness(harness, "partials")).group(1)) > 10000000


def test_slab_rule_of_the_trunk_under_the_host_sanitizers(sanitized_harness):
    run_harness(sanitized_harness, "slabs")
    run_harness(sanitized_harness, "partials")


def test_header_and_bindings_agree_on_the_new_symbols(built_lib):
    from vfa_amd import _lib
    declared = declared_parameters()
    lib = _lib.lib()
    for name, count in NEW_SYMBOLS.items():
        assert declared.get(name) == count == len(_lib.SIGNATURES[name]) and hasattr(lib, name), name
    assert _lib.ABI_VERSION == ABI_VERSION == 9 == lib.vfa_abi_version()
    assert "vfa_trunk_grad.hip" in open(built_lib.replace("libvfa_hip.so", "Makefile")).read().split("SRCS")[1]


def test_refusals_of_the_entry_points(built_lib):
    """What the calls decide before they launch anything (no device is touched: every case returns first)."""
    from vfa_amd import _lib
    lib = _lib.lib()
    assert lib.vfa_group_norm_backward_workspace_bytes(2, 64) == 2 * 64 * 32 * 2 * 8 + 1536
    assert lib.vfa_group_norm_backward_workspace_bytes(0, 64) == 0 and lib.vfa_group_norm_backward_workspace_bytes(2, 0) == 0
    p, big = ctypes.c_void_p(4096), 1 << 30       # never dereferenced
    back = lib.vfa_group_norm_backward_f32

    def call(y=p, u=p, a=p, b=p, out=p, gamma=p, stats=p, mask=0, B=1, C=64, L=3, W=5, groups=16, dy=p, dz=p, ws=p, ws_bytes=big):
        return back(y, u, a, b, out, gamma, stats, mask, B, C, L, W, groups, dy, dz, None, None, ws, ws_bytes, None)
    assert call(mask=2) == BAD and call(groups=24) == BAD and call(groups=0) == BAD and call(B=-1) == BAD
    assert call(y=None) == BAD and call(u=None) == BAD and call(stats=None) == BAD and call(dy=None) == BAD
    assert call(a=None) == BAD and call(mask=1, out=None) == BAD and call(mask=1, dz=None) == BAD
    assert call(ws=None) == BAD and call(ws_bytes=100) == BAD and call(ws=ctypes.c_void_p(4100)) == BAD
    assert call(B=70000, ws_bytes=1 << 40) == UNSUPPORTED
    stride = (ctypes.c_longlong * 4)(960, 15, 5, 1)
    stats = lib.vfa_group_norm_stats_f32
    assert stats(p, stride, p, p, 1e-5, 1, 64, 3, 5, 16, p, p, None, p, big, None) == BAD            # no stats
    assert stats(p, stride, p, p, 1e-5, 1, 64, 3, 5, 24, p, p, p, p, big, None) == BAD               # groups do not divide C
    assert stats(p, stride, p, p, 1e-5, 1, 64, 3, 5, 16, p, p, p, p, 8, None) == BAD                 # a short workspace
    per = 9 * 4
    ws, ws_heads = lib.vfa_trunk_conv_wgrad_workspace_bytes, lib.vfa_conv3x3_wgrad_workspace_bytes
    assert ws(7, 64, 64, 180, 320) == ws_heads(7, 64, 64, 180, 320) == 256 + 7 * 16 * 64 * 64 * per
    assert ws(7, 256, 256, 45, 80) == ws_heads(7, 256, 256, 45, 80) == 256 + 7 * 16 * 256 * 256 * per
    assert ws(7, 512, 512, 23, 40) == 256 + 7 * 3 * 512 * 512 * per and ws_heads(7, 512, 512, 23, 40) == 256 + 7 * 12 * 512 * 512 * per
    assert ws(2, 512, 512, 3, 5) == 256 + 2 * 512 * 512 * per and ws(0, 64, 64, 3, 5) == 0 and ws(1, 40, 64, 3, 5) == 0
    wgrad = lib.vfa_trunk_conv_wgrad_f32
    assert wgrad(p, stride, p, stride, p, None, 1, 64, 3, 5, 64, p, p, big, None) == BAD             # a without b
    assert wgrad(p, stride, p, stride, p, p, 1, 48, 3, 5, 64, p, p, big, None) == UNSUPPORTED        # C % 32
    assert wgrad(p, stride, p, stride, None, None, 1, 64, 3, 5, 64, None, p, big, None) == BAD       # no dw
    assert wgrad(p, stride, p, stride, p, p, 1, 64, 3, 5, 64, p, p, 255, None) == BAD                # a short workspace


def test_wrappers_exist_and_reject_bad_shapes():
    from vfa_amd import ops
    from vfa_amd._lib import VFAHipError
    assert list(inspect.signature(ops.group_norm_stats).parameters) == ["x", "groups", "weight", "bias", "eps"]
    assert list(inspect.signature(ops.group_norm_backward).parameters)[:7] == ["u", "y", "a", "b", "weight", "stats", "groups"]
    assert "mask_out" in inspect.signature(ops.group_norm_backward).parameters
    assert list(inspect.signature(ops.trunk_conv_input_grad).parameters) == ["grad", "weight"]
    assert list(inspect.signature(ops.trunk_conv_weight_grad).parameters) == ["grad", "x", "affine"]
    sig = inspect.signature(ops.residual_block_train)
    assert list(sig.parameters) == ["x", "w1", "g1", "b1", "w2", "g2", "b2", "groups", "eps"]
    assert sig.parameters["groups"].default == 16 and sig.parameters["eps"].default == 1e-5
    y, ga = torch.zeros(2, 64, 3, 5), torch.ones(64)
    a, stats = torch.zeros(2, 64), torch.zeros(2, 16, 2, dtype=torch.float64)
    with pytest.raises(ValueError, match="groups"):
        ops.group_norm_stats(y, 24, ga, ga, EPS)
    with pytest.raises(ValueError, match="weight / bias"):
        ops.group_norm_stats(y, 16, torch.ones(32), ga, EPS)
    with pytest.raises(ValueError, match="like y"):
        ops.group_norm_backward(torch.zeros(2, 64, 3, 6), y, a, a, ga, stats, 16)
    with pytest.raises(ValueError, match="mask_out"):
        ops.group_norm_backward(y, y, a, a, ga, stats, 16, mask_out=torch.zeros(2, 64, 5, 3))
    with pytest.raises(ValueError, match="affine"):
        ops.group_norm_backward(y, y, torch.zeros(2, 32), a, ga, stats, 16)
    with pytest.raises(ValueError, match="stats"):
        ops.group_norm_backward(y, y, a, a, ga, stats.float(), 16)
    w = torch.zeros(64, 64, 3, 3)
    with pytest.raises(ValueError, match="multiples of 32"):
        ops.trunk_conv_input_grad(y, torch.zeros(64, 40, 3, 3))
    with pytest.raises(ValueError, match="grad must be"):
        ops.trunk_conv_input_grad(torch.zeros(2, 32, 3, 5), w)
    with pytest.raises(ValueError, match="one size"):
        ops.trunk_conv_weight_grad(y, torch.zeros(2, 64, 3, 6))
    with pytest.raises(ValueError, match="multiples of 32"):
        ops.trunk_conv_weight_grad(torch.zeros(2, 40, 3, 5), y)
    with pytest.raises(ValueError, match="affine"):
        ops.trunk_conv_weight_grad(y, y, (a, torch.zeros(2, 32)))
    with pytest.raises(ValueError, match="multiple of 32"):
        ops.residual_block_train(torch.zeros(2, 40, 3, 5), w, ga, ga, w, ga, ga)
    with pytest.raises(ValueError, match="a weight"):
        ops.residual_block_train(y, w, ga, ga, torch.zeros(64, 64, 1, 1), ga, ga)
    with pytest.raises(ValueError, match="GroupNorm parameter"):
        ops.residual_block_train(y, w, ga, torch.ones(32), w, ga, ga)
    with pytest.raises(ValueError, match="groups"):
        ops.residual_block_train(y, w, ga, ga, w, ga, ga, groups=24)
    for call in (lambda: ops.residual_block_train(y, w, ga, ga, w, ga, ga), lambda: ops.group_norm_stats(y, 16, ga, ga, EPS),
                 lambda: ops.trunk_conv_input_grad(y, w), lambda: ops.trunk_conv_weight_grad(y, y),
                 lambda: ops.group_norm_backward(y, y, a, a, ga, stats, 16)):
        with pytest.raises(VFAHipError, match="CPU tensor"):      # well-formed operands: no fallback on the CPU
            call()


def _net():
    from vfa_amd.vfanet import VFANet
    return VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base="resnet18", mode="3D")


def test_trunk_convs_train_attribute():
    from vfa_amd import vfanet
    assert vfanet.TRUNK_CONVS_TRAIN == ("library", "hip")
    torch.manual_seed(3)
    net, plain = _net().train(), _net().train()
    assert net.trunk_convs_train == "library" and net.trunk_convs == "library" and net.trunk_stem == "library"
    net.trunk_convs_train = "hip"
    assert list(net.state_dict()) == list(plain.state_dict())
    plain.load_state_dict(net.state_dict())
    blocks = [b for layer in (net.base.layer1, net.base.layer2, net.base.layer3, net.base.layer4) for b in layer]
    assert [b.is_identity for b in blocks] == [True, True, False, True, False, True, False, True]
    x = torch.randn(1, 3, 64, 96)       # CPU images: the condition does not hold, the library path runs
    cot = [torch.randn(1, c, 64 // s, 96 // s) for c, s in ((128, 8), (256, 16), (512, 32))]
    got, want = net.trunk(x), plain.base(x)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    torch.autograd.backward(got, cot)
    torch.autograd.backward(want, cot)
    for (k, p), (_, q) in zip(net.base.named_parameters(), plain.base.named_parameters()):
        assert p.grad is not None and torch.equal(p.grad, q.grad), k
    net.trunk_convs_train = "fast"
    with pytest.raises(ValueError, match="trunk_convs_train"):
        net.trunk(x)


@pytest.mark.parametrize("shape", GN_SHAPES)
@pytest.mark.parametrize("with_shortcut", [False, True])
def test_restated_group_norm_backward_is_float64_autograd(shape, with_shortcut):
    B, C, L, W = shape
    y, u, r, gamma, beta = tt.gn_inputs(B, C, L, W, seed=C + L)
    shortcut = r if with_shortcut else None
    dy64, dg64, db64, dz64 = tt.gn_autograd(y, u, gamma, beta, GROUPS, EPS, torch.float64, shortcut)
    z = torch.nn.functional.group_norm(y.double(), GROUPS, gamma.double(), beta.double(), EPS)
    mask = ((z if shortcut is None else z + r.double()) > 0).numpy()
    got = tt.gn_backward_restated(y, u, mask, gamma, GROUPS, EPS)
    for what, a, b in (("dy", got["dy"], dy64), ("dgamma", got["dgamma"], dg64), ("dbeta", got["dbeta"], db64)):
        rel = cc.normwise(a, b)
        print(f"{what}: {rel:.3g}")
        assert rel < 1e-12, what
    if with_shortcut:
        assert torch.equal(got["dz"].double(), dz64)


@pytest.mark.parametrize("shape", GN_SHAPES)
def test_elementwise_yardstick_accepts_the_kernels_rounding_and_rejects_wrong_restatements(shape):
    B, C, L, W = shape
    y, u, _, gamma, beta = tt.gn_inputs(B, C, L, W, seed=C + L)
    a, b = tt.affine32(y, gamma, beta, GROUPS, EPS)
    mask = tt.mask_prologue(y, a, b)
    assert 0.2 < mask.mean() < 0.8 and (mask != (y.numpy() > 0)).mean() > 0.01
    as_kernel = tt.gn_backward_restated(y, u, mask, gamma, GROUPS, EPS, round32=True)
    tt.check_gn_elementwise(as_kernel["dy"], y, u, mask, gamma, GROUPS, EPS, "as the kernel rounds")
    for variant in ("no_q", "mask_y"):
        wrong = tt.gn_backward_restated(y, u, mask, gamma, GROUPS, EPS, round32=True, variant=variant)
        with pytest.raises(AssertionError, match=r"\(E\)"):
            tt.check_gn_elementwise(wrong["dy"], y, u, mask, gamma, GROUPS, EPS, variant)
