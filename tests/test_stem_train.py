"""Training the trunk's stem on the MI355X (``ops.stem_pool_backward``, ``ops.stem_conv_weight_grad``, ``ops.stem_train``,
``VFANet.trunk_stem_train = "hip"``) under the yardsticks of tests/stem_train_common.py.  Every shape is chosen because a kernel can
go wrong there.

Pooling backward, maps (L, W) of the raw map: 1 x 1 (one window, one tap), 2 x 3 (windows that lose a row and a column of taps), 5 x 6
and 9 x 11 (odd and even ends: a last window partly outside or not), 19 x 141 (odd on both axes, three tiles of 32 x 64 positions, the
last ones partial); C in {1, 5, 64}.  Asserted in BITS against the numpy restatement.

Weight gradient, IMAGES (L, W) under ``wgrad_slabs`` (tiles of 4 x 32 output cells, at most 64 slabs):

    1 x 1, 5 x 6, 9 x 11    one tile, one slab; a single cell, partial rows and columns, taps outside on every side
    19 x 141                output 10 x 71: 3 x 3 = 9 tiles, 9 slabs of one tile -- MORE THAN ONE SLAB, partial tiles on both axes
    72 x 512                output 36 x 256: 72 tiles in 64 slabs, so eight workgroups take TWO TILES

with O in {5, 64}, B in {1, 2}, x contiguous, channels-last and a strided slice.

Measured on the MI355X: the pooling backward equals its restatement in bits everywhere; weight gradient (N) 0.14 - 0.28 x (1.00 x on the
single-cell map); the node: out 0.97 x, dweight 0.26 x, dgamma 0.96 x, dbeta 0.28 x; the model: trunk gradients at most 1.30 x with the
stem switch alone and 2.03 x with all three (bound 4 x)."""
import copy
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch

import conv_common as cc
import stem_common as sc
import stem_train_common as st
import trunk_common as tc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
POOL_MAPS = [(1, 1), (2, 3), (5, 6), (9, 11), (19, 141)]
WGRAD_SHAPES = [(2, 1, 1), (2, 5, 6), (1, 9, 11), (2, 9, 11), (2, 19, 141), (1, 72, 512)]      # (B, L, W) of the images
PARAMS = st.PARAMS


def _bits(t):
    return t.contiguous().view(torch.int32)


def _dev(affine):
    return tuple(t.to(DEV) for t in affine)


# ---- the pooling's backward --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C", [1, 5, 64])
@pytest.mark.parametrize("L,W", POOL_MAPS)
def test_pool_backward_is_the_restatement_bit_for_bit(L, W, C):
    from vfa_amd import ops
    for integer in (False, True):
        gout, y, affine = st.pool_inputs(2, C, L, W, seed=L * W + C, integer=integer)
        assert float(affine[0].min()) < 0 < float(affine[0].max())
        want = st.emulate_pool_backward(gout, y, affine)
        u = ops.stem_pool_backward(gout.to(DEV), y.to(DEV), _dev(affine))
        assert u.shape == y.shape and u.is_contiguous()
        differ = int((_bits(u.cpu()) != _bits(want)).sum())
        print(f"pool backward {L}x{W} C={C} integer={integer}: {differ} of {u.numel()} elements differ in bits from the restatement")
        assert differ == 0
        if integer:
            st.check_pool_backward(u, gout, y, affine, f"{L}x{W} C={C}")
        alone = ops.stem_pool_backward(gout[1:].to(DEV), y[1:].to(DEV), tuple(t[1:].to(DEV) for t in affine))
        assert torch.equal(_bits(alone[0]), _bits(u[1])), "an image alone and in a batch"
        with torch.no_grad():       # the forward whose winners are recomputed: the restated taps are the forward's
            assert torch.equal(_bits(ops.stem_pool(y.to(DEV), _dev(affine)).cpu()), _bits(sc.emulate_pool(y, affine)))


def test_pool_backward_one_nan_takes_its_windows():
    from vfa_amd import ops
    gout, y, affine = st.pool_inputs(2, 5, 9, 11, seed=5, integer=False)
    y[1, 2, 4, 5] = float("nan")
    want = st.emulate_pool_backward(gout, y, affine)
    u = ops.stem_pool_backward(gout.to(DEV), y.to(DEV), _dev(affine)).cpu()
    assert not u.isnan().any() and torch.equal(_bits(u), _bits(want))
    assert float(u[1, 2, 4, 5]) == float(gout[1, 2, 2, 2] + gout[1, 2, 2, 3])


@pytest.mark.parametrize("L,W", POOL_MAPS)
def test_every_element_of_u_is_written(L, W):
    """A raw call into an output full of NaN: none is left, and the result is the wrapper's."""
    from vfa_amd import _lib, ops
    gout, y, affine = st.pool_inputs(2, 5, L, W, seed=L + W, integer=False)
    gd, yd, (ad, bd) = gout.to(DEV), y.to(DEV), _dev(affine)
    u = torch.full(y.shape, float("nan"), device=DEV)
    _lib.call("vfa_stem_pool_backward_f32", _lib.ptr(gd), _lib.ptr(yd), _lib.ptr(ad), _lib.ptr(bd), 2, 5, L, W, _lib.ptr(u), _lib.current_stream_handle())
    assert not u.isnan().any()
    assert torch.equal(_bits(u), _bits(ops.stem_pool_backward(gd, yd, (ad, bd))))


# ---- the weight gradient -----------------------------------------------------------------------------------------------------------

def _layouts(x):
    """x on the device: contiguous, channels-last, and a strided slice of a larger tensor."""
    B, C, L, W = x.shape
    big = torch.full((B, C, L + 2, 2 * W + 3), 7.0, device=DEV)
    big[:, :, 1:1 + L, 2:2 + 2 * W:2] = x.to(DEV)
    view = big[:, :, 1:1 + L, 2:2 + 2 * W:2]
    assert not view.is_contiguous() and view.stride(3) == 2
    return {"contiguous": x.to(DEV), "channels-last": x.to(DEV).to(memory_format=torch.channels_last), "slice": view}


@pytest.mark.parametrize("O", [5, 64])
@pytest.mark.parametrize("B,L,W", WGRAD_SHAPES)
def test_weight_gradient_of_integer_operands_is_exact(B, L, W, O):
    """Values in {-2 .. 2}: a product is an integer of magnitude <= 4 and a sum over B Lo Wo <= 9216 cells stays below 2^24, so every
    float32 partial, the float64 merge and its rounding are exact: dw must EQUAL float64 -- every tap, border, tile and slab."""
    from vfa_amd import ops
    g, x = st.wgrad_inputs(B, O, L, W, seed=L + W + O, integer=True)
    assert B * sc.out_size(L) * sc.out_size(W) * 4 < 2 ** 24
    dw64 = st.wgrad(g, x, torch.float64)
    for name, xd in _layouts(x).items():
        dw = ops.stem_conv_weight_grad(g.to(DEV), xd)
        assert dw.shape == (O, 3, 7, 7) and dw.is_contiguous()
        differ = int((dw.cpu().double() != dw64).sum())
        print(f"dW integer B={B} {L}x{W} O={O} {name}: {differ} of {dw.numel()} elements differ from float64")
        assert differ == 0, name


@pytest.mark.parametrize("O", [5, 64])
@pytest.mark.parametrize("B,L,W", WGRAD_SHAPES)
def test_weight_gradient_of_random_operands(B, L, W, O):
    from vfa_amd import ops
    g, x = st.wgrad_inputs(B, O, L, W, seed=L + W + O)
    dw64, dw32 = st.wgrad(g, x, torch.float64), st.wgrad(g, x, torch.float32)
    dw = ops.stem_conv_weight_grad(g.to(DEV), x.to(DEV))
    cc.check_normwise(dw, dw64, dw32, f"dW B={B} {L}x{W} O={O}")
    assert torch.equal(_bits(dw), _bits(ops.stem_conv_weight_grad(g.to(DEV), x.to(DEV)))), "two runs"
    last = ops.stem_conv_weight_grad(g.to(DEV), x.to(DEV).to(memory_format=torch.channels_last))
    cc.check_normwise(last, dw64, dw32, f"dW B={B} {L}x{W} O={O} channels-last")


def test_the_yardstick_sees_an_index_error():
    g, x = st.wgrad_inputs(2, 64, 19, 141, seed=11)
    dw64, dw32 = st.wgrad(g, x, torch.float64), st.wgrad(g, x, torch.float32)
    cc.check_normwise(st.emulate_wgrad(g, x), dw64, dw32, "restated dW")
    with pytest.raises(AssertionError):
        cc.check_normwise(st.emulate_wgrad(g, x, pad=2), dw64, dw32, "padding 2")
    with pytest.raises(AssertionError):
        cc.check_normwise(st.emulate_wgrad(g, x, swap=True), dw64, dw32, "ky and kx exchanged")


def test_empty_batch_gives_zeros():
    from vfa_amd import ops
    dw = ops.stem_conv_weight_grad(torch.zeros(0, 64, 5, 6, device=DEV), torch.zeros(0, 3, 9, 11, device=DEV))
    assert dw.shape == (64, 3, 7, 7) and not dw.any()


# ---- the node ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _trunk_case():
    from vfa_amd.vfanet import _DEPTHS, _Trunk
    torch.manual_seed(31)
    trunk = tc.randomise_group_norms(_Trunk(_DEPTHS["resnet18"]), 32).train()
    gen = torch.Generator().manual_seed(33)
    x = torch.randn(2, 3, 37, 139, generator=gen)      # raw map 19 x 70, pooled 10 x 35
    x[1] *= 1.7
    g = torch.randn(2, 64, 10, 35, generator=gen)
    return trunk, x, g


def _node_step(trunk, x, g, frozen=()):
    trunk = copy.deepcopy(trunk).to(DEV)
    for k in frozen:
        dict(trunk.named_parameters())[k].requires_grad_(False)
    out = trunk.stem_train_hip(x.to(DEV))
    out.backward(g.to(DEV))
    return out.detach(), {k: dict(trunk.named_parameters())[k].grad for k in PARAMS}


def test_node_forward_is_stem_hip_and_gradients_meet_the_yardstick():
    trunk, x, g = _trunk_case()
    out, grads = _node_step(trunk, x, g)
    with torch.no_grad():
        want = copy.deepcopy(trunk).to(DEV).stem_hip(x.to(DEV))
    assert out.is_contiguous() and torch.equal(_bits(out), _bits(want)), "the forward is stem_hip's"
    out64, grads64 = st.stem_step(trunk, x, g, torch.float64)
    out32, grads32 = st.stem_step(trunk, x, g, torch.float32)
    cc.check_normwise(out, out64, out32, "stem out")
    for k in PARAMS:
        cc.check_normwise(grads[k], grads64[k], grads32[k], f"stem d {k}")
    out2, grads2 = _node_step(trunk, x, g)
    assert all(torch.equal(_bits(grads[k]), _bits(grads2[k])) for k in PARAMS), "two runs"


def test_node_launches_only_what_is_needed():
    from vfa_amd import ops
    trunk, x, g = _trunk_case()
    _, grads = _node_step(trunk, x, g)
    with ops.KernelTimer() as kt:
        _, frozen = _node_step(trunk, x, g, frozen=("conv1.weight",))
    torch.cuda.synchronize()
    seen = kt.summary()
    assert "vfa_stem_conv_wgrad_f32" not in seen
    assert seen["vfa_stem_pool_backward_f32"]["launches"] == 1 and seen["vfa_group_norm_backward_f32"]["launches"] == 1
    assert frozen["conv1.weight"] is None
    assert all(torch.equal(_bits(frozen[k]), _bits(grads[k])) for k in PARAMS[1:])
    with ops.KernelTimer() as kt:
        _node_step(trunk, x, g)
    torch.cuda.synchronize()
    assert kt.summary()["vfa_stem_conv_wgrad_f32"]["launches"] == 1
    with pytest.raises(ValueError, match="requires grad"):
        copy.deepcopy(trunk).to(DEV).stem_train_hip(x.to(DEV).requires_grad_())


def _saved_bytes(run, skip):
    """The bytes of the distinct tensors an autograd graph saves, the parameters themselves (``skip``) left out."""
    seen = {}

    def pack(t):
        if t.data_ptr() not in skip:
            seen[t.data_ptr()] = max(seen.get(t.data_ptr(), 0), t.numel() * t.element_size())
        return t
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = run()
    return sum(seen.values()), out


def test_node_saves_the_images_and_one_raw_map():
    """What the design keeps: x, the raw map, (a, b) and the statistics -- no normalised map, no index map (no winner bytes: the
    winners are recomputed).  The library chain on the same input keeps more."""
    trunk, x, g = _trunk_case()
    dev = copy.deepcopy(trunk).to(DEV)
    xd = x.to(DEV)
    skip = {p.data_ptr() for p in dev.parameters()}
    B, O, Lo, Wo = 2, 64, 19, 70
    bound = xd.numel() * 4 + B * O * Lo * Wo * 4 + 2 * B * O * 4 + B * dev.bn1.num_groups * 2 * 8
    mine, _ = _saved_bytes(lambda: dev.stem_train_hip(xd), skip)
    library, _ = _saved_bytes(lambda: dev.stem(xd), skip)
    print(f"saved for backward: hip {mine} bytes (bound {bound}), library {library} bytes")
    assert mine <= bound < library


def test_node_graph_replay_equals_the_eager_step():
    trunk, x, g = _trunk_case()
    out, grads = _node_step(trunk, x, g)
    dev = copy.deepcopy(trunk).to(DEV)
    params = [dict(dev.named_parameters())[k] for k in PARAMS]
    xs, gs = x.to(DEV), g.to(DEV).clone()

    def step():
        o = dev.stem_train_hip(xs)
        return (o.detach(), *torch.autograd.grad(o, params, gs))
    side = torch.cuda.Stream(device=DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream(DEV).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(captured, (out, *(grads[k] for k in PARAMS))):
        assert torch.equal(_bits(a), _bits(b))


# ---- the model ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _net_and_references():
    from vfa_amd.vfanet import VFANet
    torch.manual_seed(41)
    net = VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base="resnet18", mode="3D").train()
    tc.randomise_group_norms(net.base, 42)
    gen = torch.Generator().manual_seed(43)
    x = torch.randn(2, 3, 64, 96, generator=gen)
    x[1] *= 1.5
    cot = tuple(torch.randn(2, c, 64 // s, 96 // s, generator=gen) for c, s in ((128, 8), (256, 16), (512, 32)))
    ref64 = st.trunk_step(copy.deepcopy(net).double(), x.double(), cot)
    ref32 = st.trunk_step(net, x, cot)
    return net, x, cot, ref64, ref32


def _switched(net, all_three):
    dev = copy.deepcopy(net).to(DEV)
    dev.trunk_stem_train = "hip"
    if all_three:
        dev.trunk_convs_train = dev.trunk_proj_train = "hip"
    ran = []
    dev.base.conv1.register_forward_hook(lambda *_: ran.append("conv1"))
    dev.base.bn1.register_forward_hook(lambda *_: ran.append("bn1"))
    return dev, ran


@pytest.mark.parametrize("all_three", [False, True])
def test_model_against_the_float64_model(all_three):
    net, x, cot, (maps64, grads64), (maps32, grads32) = _net_and_references()
    dev, ran = _switched(net, all_three)
    maps, grads = st.trunk_step(dev, x.to(DEV), cot)
    assert list(dev.state_dict()) == list(net.state_dict()) and sorted(grads) == sorted(grads64)
    for name, m, m64, m32 in zip(("f8", "f16", "f32"), maps, maps64, maps32):
        cc.check_normwise(m, m64, m32, f"map {name}")
    worst = 0.0
    for k in sorted(grads):
        assert grads[k] is not None, k
        worst = max(worst, cc.check_normwise(grads[k], grads64[k], grads32[k], f"d {k}")[2])
    print(f"model (all three switches: {all_three}): the worst (N) ratio of a trunk gradient is {worst:.2f} x")


def test_model_stem_does_not_run_as_a_module():
    net, x, cot, _, _ = _net_and_references()
    dev, ran = _switched(net, True)
    maps = dev.trunk(x.to(DEV))
    torch.autograd.backward(maps, [c.to(DEV) for c in cot])
    assert ran == [] and dev.base.conv1.weight.grad is not None


def test_model_gives_the_same_bits_twice_without_the_deterministic_setting():
    assert not torch.are_deterministic_algorithms_enabled()
    net, x, cot, _, _ = _net_and_references()
    dev, _ = _switched(net, True)
    (_, first), (_, second) = st.trunk_step(dev, x.to(DEV), cot), st.trunk_step(dev, x.to(DEV), cot)
    assert len(first) > 50 and "conv1.weight" in first and "bn1.weight" in first and "bn1.bias" in first
    for k in first:
        assert torch.equal(_bits(first[k]), _bits(second[k])), k


def test_an_input_that_requires_grad_takes_the_module_stem():
    net, x, cot, _, _ = _net_and_references()
    dev, ran = _switched(net, True)
    xd = x.to(DEV).requires_grad_()
    maps = dev.trunk(xd)
    torch.autograd.backward(maps, [c.to(DEV) for c in cot])
    assert ran == ["conv1", "bn1"]
    assert xd.grad is not None and float(xd.grad.abs().max()) > 0
    assert all(p.grad is not None for p in dev.base.parameters())
