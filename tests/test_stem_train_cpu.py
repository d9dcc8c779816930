"""The stem's training path without a GPU: the integer rules of the two backward kernels (vfa_amd/csrc/vfa_stem.h) compiled with g++
into tests/native/stem_grad_harness.cpp and checked against brute force, once more under the host sanitizers; the numpy restatement
of the pooling's backward (tests/stem_train_common.py) against float64 autograd on tie-rich integer input, with two wrong restatements
failing on the same input; the restated weight gradient under (N), with two wrong restatements failing; what the entry points refuse
before they launch; the switch ``VFANet.trunk_stem_train`` and the ABI."""
import ctypes
import inspect
import re
from types import SimpleNamespace

import pytest
import torch

import conv_common as cc
import stem_common as sc
import stem_train_common as st
from native_common import build_harness, declared_parameters, run_harness

GXX_FLAGS = ["-O1", "-std=c++17", "-Wall"]
BAD, UNSUPPORTED = 10001, 10002
NEW_SYMBOLS = ("vfa_stem_pool_backward_f32", "vfa_stem_conv_wgrad_workspace_bytes", "vfa_stem_conv_wgrad_f32")


@pytest.fixture(scope="module")
def built_lib():
    from vfa_amd import build
    return build.build()


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "stem_grad", "stem_grad_harness.cpp", GXX_FLAGS)


@pytest.fixture(scope="module")
def sanitized_harness(tmp_path_factory):
    return build_harness(tmp_path_factory, "stem_grad", "stem_grad_harness.cpp", GXX_FLAGS, sanitized=True)


def test_windows_that_contain_a_position_against_the_enumeration(harness):
    assert int(re.search(r"(\d+) positions", run_harness(harness, "windows")).group(1)) == 300 * 301 // 2


def test_scan_order_of_a_windows_taps_against_the_enumeration(harness):
    assert int(re.search(r"(\d+) taps", run_harness(harness, "scan")).group(1)) > 1000000


def test_slab_rule_against_the_enumeration(harness):
    out = run_harness(harness, "slabs")
    n_slabs, cells = (int(v) for v in re.findall(r"(\d+) (?:slabs|cells)", out))
    assert n_slabs > 3000 and cells > 100000


def test_integer_rules_under_the_host_sanitizers(sanitized_harness):
    for mode in ("windows", "scan", "slabs"):
        run_harness(sanitized_harness, mode)


@pytest.mark.parametrize("L,W", [(1, 1), (2, 3), (5, 6), (9, 11), (19, 141)])
def test_restated_pool_backward_equals_float64_autograd_and_two_wrong_rules_fail(L, W):
    gout, y, affine = st.pool_inputs(2, 5, L, W, seed=L * W, integer=True)
    assert float(affine[0].min()) < 0 < float(affine[0].max())
    u = st.emulate_pool_backward(gout, y, affine)
    assert u.shape == y.shape and u.dtype == torch.float32
    st.check_pool_backward(u, gout, y, affine, f"restated {L}x{W}")
    assert torch.equal(u[1], st.emulate_pool_backward(gout[1:], y[1:], (affine[0][1:], affine[1][1:]))[0])      # per image
    if L * W >= 30:     # (smaller maps have too few ties and borders to tell the rules apart)
        with pytest.raises(AssertionError, match="masked elements differ"):
            st.check_pool_backward(st.emulate_pool_backward(gout, y, affine, last_wins=True), gout, y, affine, "the last maximum wins")
        with pytest.raises(AssertionError, match="outside the map"):
            st.check_pool_backward(st.emulate_pool_backward(gout, y, affine, outside_zero=True), gout, y, affine, "zeros outside the map win")


def test_a_nan_takes_its_windows_in_the_restatement():
    """The last NaN in scan order wins; one NaN wins every window that holds it (position (4, 5): windows (2, 2) and (2, 3))."""
    gout, y, affine = st.pool_inputs(1, 2, 9, 11, seed=3, integer=False)
    y[0, 1, 4, 5] = float("nan")
    u = st.emulate_pool_backward(gout, y, affine)
    assert not u.isnan().any()
    assert float(u[0, 1, 4, 5]) == float(gout[0, 1, 2, 2] + gout[0, 1, 2, 3])
    assert torch.equal(u[0, 0], st.emulate_pool_backward(gout[:, :1], y[:, :1], (affine[0][:, :1], affine[1][:, :1]))[0, 0])


@pytest.mark.parametrize("O,L,W", [(64, 9, 11), (5, 19, 141), (64, 1, 1)])
def test_restated_weight_gradient_meets_the_yardstick_and_two_wrong_restatements_fail(O, L, W):
    g, x = st.wgrad_inputs(2, O, L, W, seed=O + L + W)
    dw64, dw32 = st.wgrad(g, x, torch.float64), st.wgrad(g, x, torch.float32)
    cc.check_normwise(st.emulate_wgrad(g, x), dw64, dw32, f"restated dW O={O} {L}x{W}")
    if L > 1:
        with pytest.raises(AssertionError):
            cc.check_normwise(st.emulate_wgrad(g, x, pad=2), dw64, dw32, "padding 2")
        with pytest.raises(AssertionError):
            cc.check_normwise(st.emulate_wgrad(g, x, swap=True), dw64, dw32, "ky and kx exchanged")


def test_abi_and_signatures():
    from vfa_amd import _lib
    import native_common
    assert _lib.ABI_VERSION == 9 == native_common.ABI_VERSION
    declared = declared_parameters()
    for name in NEW_SYMBOLS:
        assert name in _lib.SIGNATURES and declared[name] == len(_lib.SIGNATURES[name]), name
    assert len(_lib.SIGNATURES["vfa_stem_pool_backward_f32"]) == 10 and len(_lib.SIGNATURES["vfa_stem_conv_wgrad_f32"]) == 11


def test_refusals_of_the_entry_points(built_lib):
    """What the calls decide before they launch anything (no device is touched: every case returns first)."""
    from vfa_amd import _lib
    lib = _lib.lib()
    tiles, slabs = st.slabs(19, 141)
    assert (tiles, slabs) == (9, 9) and st.slabs(72, 512) == (72, 64) and st.slabs(720, 1280) == (1800, 64)
    assert lib.vfa_stem_conv_wgrad_workspace_bytes(2, 5, 19, 141) == 2 * 9 * 5 * 147 * 4
    assert lib.vfa_stem_conv_wgrad_workspace_bytes(7, 64, 720, 1280) == 7 * 64 * 64 * 147 * 4
    for bad in ((0, 64, 8, 8), (1, 0, 8, 8), (1, 65, 8, 8), (1, 64, 0, 8), (1, 64, 8, -1), (70000, 64, 8, 8)):
        assert lib.vfa_stem_conv_wgrad_workspace_bytes(*bad) == 0
    stride = (ctypes.c_longlong * 4)(3 * 16, 16, 4, 1)
    negative = (ctypes.c_longlong * 4)(3 * 16, 16, -4, 1)
    huge = (ctypes.c_longlong * 4)(1 << 40, 1 << 31, 4, 1)
    p = ctypes.c_void_p(4096)   # (never dereferenced)
    ws_bytes = 64 * 147 * 4

    def wgrad(B=1, L=4, W=4, O=64, g=p, x=p, stride=stride, dw=p, ws=p, ws_bytes=ws_bytes):
        return lib.vfa_stem_conv_wgrad_f32(g, x, stride, B, L, W, O, dw, ws, ws_bytes, None)

    def pool(B=1, C=64, L=4, W=4, gout=p, y=p, a=p, b=p, u=p):
        return lib.vfa_stem_pool_backward_f32(gout, y, a, b, B, C, L, W, u, None)

    for call in (wgrad, pool):
        assert call(B=-1) == BAD and call(L=-1) == BAD and call(W=-1) == BAD
        assert call(B=70000) == UNSUPPORTED and call(L=70000) == UNSUPPORTED and call(L=1 << 15, W=1 << 15) == UNSUPPORTED
    assert wgrad(O=0) == BAD and wgrad(dw=None) == BAD and wgrad(g=None) == BAD and wgrad(x=None) == BAD and wgrad(stride=None) == BAD
    assert wgrad(stride=negative) == BAD and wgrad(ws=None) == BAD and wgrad(ws_bytes=ws_bytes - 1) == BAD and wgrad(ws=ctypes.c_void_p(4100)) == BAD
    assert wgrad(O=65) == UNSUPPORTED and wgrad(stride=huge) == UNSUPPORTED
    assert pool(C=-1) == BAD and pool(gout=None) == BAD and pool(y=None) == BAD and pool(a=None) == BAD and pool(b=None) == BAD and pool(u=None) == BAD
    assert pool(B=65535, C=65535) == UNSUPPORTED
    assert pool(B=0) == 0 and pool(C=0) == 0 and pool(L=0) == 0 and pool(W=0) == 0          # empty: u is not written


def _net(base="resnet18", mode="2D"):
    from vfa_amd.vfanet import VFANet
    return VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base=base, mode=mode)


def test_trunk_stem_train_attribute():
    from vfa_amd import vfanet
    assert vfanet.TRUNK_STEM_TRAIN == ("library", "hip")
    net = _net()
    assert net.trunk_stem_train == "library" and "trunk_stem_train" not in net.state_dict()
    assert (net.trunk_stem, net.trunk_convs, net.trunk_convs_train, net.trunk_proj_train, net.head_convs, net.head_convs_train) == ("library",) * 6
    x = torch.randn(1, 3, 32, 32)
    for bad in ("miopen", "", 1, None):
        net.trunk_stem_train = bad
        with pytest.raises(ValueError, match="trunk_stem_train"):
            net.trunk(x)
        with pytest.raises(ValueError, match="trunk_stem_train"):
            net.laterals(x)
    net.trunk_stem_train, net.trunk_proj_train = "hip", "nothing"
    with pytest.raises(ValueError, match="trunk_proj_train"):          # each bad value is named by its own attribute
        net.trunk(x)
    net.trunk_proj_train = "library"


def test_on_the_cpu_every_setting_is_the_module_trunk(monkeypatch):
    from vfa_amd import ops
    net = _net()
    x = torch.randn(1, 3, 32, 32)
    want = net.base(x)

    def never(*args, **kwargs):
        raise AssertionError("a HIP training node was called on a CPU tensor")
    for name in ("stem_train", "residual_block_train", "projection_block_train"):
        monkeypatch.setattr(ops, name, never)
    for stem in ("library", "hip"):
        for convs in ("library", "hip"):
            for proj in ("library", "hip"):
                net.trunk_stem_train, net.trunk_convs_train, net.trunk_proj_train = stem, convs, proj
                for mode in (net.train, net.eval):
                    mode()
                    got = net.trunk(x)
                    assert all(torch.equal(g, w) for g, w in zip(got, want))
                got_grads = torch.autograd.grad([m.sum() for m in got], [net.base.conv1.weight, net.base.bn1.weight])
                assert all(g is not None and bool(g.abs().sum() > 0) for g in got_grads)
    with torch.no_grad():
        assert all(torch.equal(g, w) for g, w in zip(net.trunk(x), want))


def test_state_dict_keys_do_not_change():
    for base in ("resnet18", "resnet34"):
        a, b = _net(base), _net(base)
        b.trunk_stem_train = "hip"
        assert list(a.state_dict()) == list(b.state_dict())
        assert [n for n, _ in a.named_modules()] == [n for n, _ in b.named_modules()]


def test_wrappers_validate_and_refuse_cpu_tensors(built_lib):
    from vfa_amd import ops
    from vfa_amd._lib import VFAHipError
    assert list(inspect.signature(ops.stem_pool_backward).parameters) == ["gout", "y", "affine"]
    assert list(inspect.signature(ops.stem_conv_weight_grad).parameters) == ["grad", "x"]
    assert list(inspect.signature(ops.stem_train).parameters) == ["x", "weight", "gamma", "beta", "groups", "eps"]
    x, w, gamma = torch.zeros(1, 3, 8, 8), torch.zeros(64, 3, 7, 7), torch.ones(64)
    y, ab, gout, g = torch.zeros(1, 64, 4, 4), (torch.ones(1, 64), torch.zeros(1, 64)), torch.zeros(1, 64, 2, 2), torch.zeros(1, 64, 4, 4)
    for call in (lambda: ops.stem_pool_backward(gout, y, ab), lambda: ops.stem_conv_weight_grad(g, x), lambda: ops.stem_train(x, w, gamma, gamma)):
        with pytest.raises(VFAHipError):
            call()
    with pytest.raises(ValueError, match="requires grad"):
        ops.stem_train(x.clone().requires_grad_(), w, gamma, gamma)
    for call in (lambda: ops.stem_train(x.double(), w, gamma, gamma), lambda: ops.stem_train(x[:, :2], w, gamma, gamma),
                 lambda: ops.stem_train(x, torch.zeros(65, 3, 7, 7), gamma, gamma), lambda: ops.stem_train(x, w, gamma[:32], gamma),
                 lambda: ops.stem_train(x, w, gamma, gamma, groups=5)):
        with pytest.raises(ValueError, match="stem_train"):
            call()
