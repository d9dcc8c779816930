"""Training the trunk's projection blocks on the MI355X (``ops.trunk_down_weight_grad``, ``ops.trunk_down_input_grad``,
``ops.projection_block_train``, ``VFANet.trunk_proj_train = "hip"``) against float64 autograd on the CPU, under the yardsticks of
tests/trunk_proj_common.py: (N) normwise within 4 x the float32 autograd chain on the CPU, (E) the elementwise bound of the weight
gradient.  Shapes (B, C, O, L, W) of x:

    (2, 64, 128, 9, 13)    L and W odd: the last tap row and column fall outside the map
    (1, 64, 128, 8, 13)    L even, W odd
    (1, 256, 512, 6, 10)   even sizes; two accumulator chains in the input gradient; slabs_for past 256^2
    (2, 128, 256, 16, 66)  g is 8 x 33: two column tiles, two row tiles, several slabs
    (1, 64, 128, 1, 1)     the odd classes are empty, a single cell
    (1, 64, 128, 2, 2)     a single output cell reached from four input positions

Asserted in bits: two runs, an image alone against the batch, integer-valued operands against float64 (every tap, parity and border
without a tolerance), the block's forward against ``_Block.forward_hip``, frozen weights, the graph replay.  Every test prints its
measured ratios before it asserts.

Measured on the MI355X: weight gradient (E) 0.07 - 11 % of the bound and 64 % on the two single-cell maps (n = 12), (N) 0.32 - 1.45 x
and 3.2 - 3.9 x on the single-cell maps (the library's side is one rounding of one product there); input gradient (N) 0.59 - 1.15 x;
the blocks: out 1.40 x and 1.75 x, dx 1.01 x and 0.87 x, parameter gradients 0.30 - 2.38 x; the model with both switches: maps
1.27 - 1.75 x, trunk parameter gradients 0.53 - 2.08 x."""
import copy
import ctypes
import functools
from types import SimpleNamespace

import pytest
import torch

import conv_common as cc
import trunk_common as tc
import trunk_proj_common as tp

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
BLOCK_SHAPES = {(64, 128): (2, 64, 12, 40), (256, 512): (2, 256, 6, 10)}
PARAMS = tp.PARAMS


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _case(shape, kernel):
    B, C, O, L, W = shape
    return tp.inputs(B, C, O, L, W, seed=C + L + W, kernel=kernel)


@pytest.mark.parametrize("kernel", [3, 1])
@pytest.mark.parametrize("shape", tp.SHAPES)
def test_weight_gradient(shape, kernel):
    from vfa_amd import ops
    B, C, O, L, W = shape
    x, _, g = _case(shape, kernel)
    dw = ops.trunk_down_weight_grad(g.to(DEV), x.to(DEV), kernel)
    assert dw.shape == (O, C, kernel, kernel) and dw.is_contiguous()
    tp.check_wgrad(dw, g, x, kernel, f"{shape} dW {kernel} x {kernel}")
    assert torch.equal(_bits(dw), _bits(ops.trunk_down_weight_grad(g.to(DEV), x.to(DEV), kernel)))
    if kernel == 1:                                            # the centre tap of the stride-1 kernel on the materialised view
        view = x[:, :, ::2, ::2].contiguous()
        centre = ops.trunk_conv_weight_grad(g.to(DEV), view.to(DEV))[:, :, 1:2, 1:2]
        tp.check_wgrad(centre, g, x, 1, f"{shape} the centre tap on the view")
        strided = ops.trunk_down_weight_grad(g.to(DEV), x.to(DEV).to(memory_format=torch.channels_last), 1)   # read through the strides
        tp.check_wgrad(strided, g, x, 1, f"{shape} channels-last x")


@pytest.mark.parametrize("shape", tp.SHAPES)
def test_input_gradient(shape):
    from vfa_amd import ops
    B, C, O, L, W = shape
    x, w, g = _case(shape, 3)
    dx = ops.trunk_down_input_grad(g.to(DEV), w.to(DEV), (L, W))
    assert dx.shape == x.shape and dx.is_contiguous()
    cc.check_normwise(dx, tp.grads(x, w, g, torch.float64)[0], tp.grads(x, w, g, torch.float32)[0], f"{shape} dX")
    assert torch.equal(_bits(dx), _bits(ops.trunk_down_input_grad(g.to(DEV), w.to(DEV), (L, W))))
    alone = ops.trunk_down_input_grad(g[:1].to(DEV), w.to(DEV), (L, W))
    assert torch.equal(_bits(alone[0]), _bits(dx[0]))
    base = torch.randn(x.shape, generator=torch.Generator().manual_seed(6)).to(DEV) * dx.abs().max()
    added = ops.trunk_down_input_grad(g.to(DEV), w.to(DEV), (L, W), add_to=base.clone())      # base + gradient: one float32 addition
    assert torch.equal(_bits(added), _bits(base + dx))


@pytest.mark.parametrize("shape", tp.SHAPES)
def test_projection_term_is_added_to_the_even_positions(shape):
    """The 1 x 1 weight's input gradient exists as the second term of a sum: base + term, one rounding of each."""
    from vfa_amd import ops
    B, C, O, L, W = shape
    x, w, g = _case(shape, 1)
    base = torch.randn(x.shape, generator=torch.Generator().manual_seed(5)) * float(g.abs().max() * w.abs().max())
    got = ops.trunk_down_input_grad(g.to(DEV), w.to(DEV), (L, W), add_to=base.to(DEV).clone())
    odd = torch.ones(L, W, dtype=torch.bool)
    odd[::2, ::2] = False
    assert torch.equal(_bits(got.cpu()[:, :, odd]), _bits(base[:, :, odd])), "only the even positions are touched"
    cc.check_normwise(got, base.double() + tp.grads(x, w, g, torch.float64)[0], base + tp.grads(x, w, g, torch.float32)[0],
                      f"{shape} base + the projection's term")
    again = ops.trunk_down_input_grad(g.to(DEV), w.to(DEV), (L, W), add_to=base.to(DEV).clone())
    assert torch.equal(_bits(got), _bits(again))


@pytest.mark.parametrize("shape", tp.SHAPES)
def test_integer_operands_are_exact(shape):
    """g, w and x hold integers of magnitude <= 4 and a 4 in every image, so every scale is 2^12: a scaled value is k 2^12 with
    |k| <= 4, one fp16 piece (the low piece is zero).  A product of two pieces is an integer multiple of 2^24 below 2^28 and every
    partial sum of at most 4 * 4 * 9 * 512 = 73 728 of them (the input gradient; B Lo Wo <= 528 cells in the weight gradient) is an
    integer below 2^24 times 2^24: float32 holds each exactly, the unscaling by 2^-24 is exact, and so are the float64 merge and
    its rounding.  Both kernels must EQUAL float64: every tap, parity and border without a tolerance."""
    from vfa_amd import ops
    B, C, O, L, W = shape
    for kernel in (3, 1):
        x, w, g = tp.integer_inputs(B, C, O, L, W, seed=L + W, kernel=kernel)
        dx64, dw64 = tp.grads(x, w, g, torch.float64)
        dw = ops.trunk_down_weight_grad(g.to(DEV), x.to(DEV), kernel)
        assert torch.equal(dw.cpu().double(), dw64), f"dW {kernel} x {kernel}: {int((dw.cpu().double() != dw64).sum())} elements differ"
        if kernel == 3:
            dx = ops.trunk_down_input_grad(g.to(DEV), w.to(DEV), (L, W))
        else:
            dx = ops.trunk_down_input_grad(g.to(DEV), w.to(DEV), (L, W), add_to=torch.zeros(x.shape, device=DEV))
        assert torch.equal(dx.cpu().double(), dx64), f"dX {kernel} x {kernel}: {int((dx.cpu().double() != dx64).sum())} elements differ"


@pytest.mark.parametrize("shape", tp.SHAPES)
def test_every_element_of_dx_is_written(shape):
    """A raw call into an output full of NaN: none is left, and the result is the wrapper's."""
    from vfa_amd import _lib, ops
    B, C, O, L, W = shape
    x, w, g = _case(shape, 3)
    gd, wd = g.to(DEV), w.to(DEV)
    dx = torch.full(x.shape, float("nan"), device=DEV)
    ws_bytes = _lib.lib().vfa_trunk_down_dgrad_workspace_bytes(B, O, C, 3)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    _lib.call("vfa_trunk_down_dgrad_f32", _lib.ptr(gd), (ctypes.c_longlong * 4)(*gd.stride()), _lib.ptr(wd), B, O, gd.shape[2], gd.shape[3], C, L, W,
              3, 0, _lib.ptr(dx), _lib.ptr(ws), ws_bytes, _lib.current_stream_handle())
    assert not dx.isnan().any()
    assert torch.equal(_bits(dx), _bits(ops.trunk_down_input_grad(gd, wd, (L, W))))


# ---- the block -------------------------------------------------------------------------------------------------------------------

def _block_step(block, x, g, frozen=False):
    """forward + backward of ``_Block.forward_train_hip`` on fresh leaves of a copy -> (out, dx, {parameter: gradient})."""
    block = copy.deepcopy(block).to(DEV).requires_grad_(not frozen)
    xd = x.to(DEV).requires_grad_()
    out = block.forward_train_hip(xd)
    out.backward(g.to(DEV))
    return out.detach(), xd.grad, {k: p.grad for k, p in block.named_parameters()}


@functools.lru_cache(maxsize=None)
def _block_case(pair):
    B, _, L, W = BLOCK_SHAPES[pair]
    block = tp.block_of(*pair, seed=pair[0])
    x, g = tp.block_inputs(block, B, L, W, seed=pair[0] + 3)
    return block, x, g, _block_step(block, x, g)


@pytest.mark.parametrize("pair", list(BLOCK_SHAPES))
def test_block_against_the_float64_module(pair):
    import trunk_train_common as tt
    block, x, g, (out, dx, grads) = _block_case(pair)
    with torch.no_grad():
        want = copy.deepcopy(block).to(DEV).forward_hip(x.to(DEV))
    assert out.is_contiguous() and torch.equal(_bits(out), _bits(want)), "the forward is forward_hip's"
    out64, dx64, grads64 = tp.block_restated(block, x, g)
    out32, dx32, grads32 = tt.block_step(block, x, g, torch.float32)
    assert sorted(grads) == sorted(PARAMS)
    cc.check_normwise(out, out64, out32, f"{pair} out")
    cc.check_normwise(dx, dx64, dx32, f"{pair} dx")
    for k in PARAMS:
        cc.check_normwise(grads[k], grads64[k].reshape(grads[k].shape), grads32[k], f"{pair} d {k}")


@pytest.mark.parametrize("pair", list(BLOCK_SHAPES))
def test_block_bits(pair):
    """Two runs without torch's deterministic setting, image 0 alone, frozen weights."""
    assert not torch.are_deterministic_algorithms_enabled()
    block, x, g, (out, dx, grads) = _block_case(pair)
    out2, dx2, grads2 = _block_step(block, x, g)
    assert torch.equal(_bits(out), _bits(out2)) and torch.equal(_bits(dx), _bits(dx2))
    for k in PARAMS:
        assert torch.equal(_bits(grads[k]), _bits(grads2[k])), k
    assert float(dx.abs().max()) > 0
    _, dx_alone, _ = _block_step(block, x[:1], g[:1])
    assert torch.equal(_bits(dx_alone[0]), _bits(dx[0]))
    _, dx_frozen, none = _block_step(block, x, g, frozen=True)
    assert all(v is None for v in none.values()) and torch.equal(_bits(dx_frozen), _bits(dx))


def test_block_launches_only_what_is_needed():
    """Frozen weights: no weight gradient is launched; x without a gradient: no stride-2 input gradient."""
    from vfa_amd import ops
    block, x, g, (_, dx, grads) = _block_case((64, 128))
    with ops.KernelTimer() as kt:
        _block_step(block, x, g, frozen=True)
    torch.cuda.synchronize()
    seen = kt.summary()
    assert "vfa_trunk_conv_wgrad_f32" not in seen and "vfa_trunk_down_wgrad_f32" not in seen
    assert seen["vfa_trunk_down_dgrad_f32"]["launches"] == 2 and seen["vfa_group_norm_backward_f32"]["launches"] == 3
    dev = copy.deepcopy(block).to(DEV)
    with ops.KernelTimer() as kt:
        dev.forward_train_hip(x.to(DEV)).backward(g.to(DEV))       # x needs no gradient
    torch.cuda.synchronize()
    seen = kt.summary()
    assert "vfa_trunk_down_dgrad_f32" not in seen
    assert seen["vfa_trunk_down_wgrad_f32"]["launches"] == 2 and seen["vfa_trunk_conv_wgrad_f32"]["launches"] == 1
    for k, p in dev.named_parameters():
        assert torch.equal(_bits(p.grad), _bits(grads[k])), k


def test_block_graph_replay_equals_the_eager_step():
    """One forward + backward: a single chain on the capture stream, the default queue count."""
    block, x, g, (out, dx, grads) = _block_case((64, 128))
    dev = copy.deepcopy(block).to(DEV)
    params = [dict(dev.named_parameters())[k] for k in PARAMS]
    xs, gs = x.to(DEV).requires_grad_(), g.to(DEV).clone()

    def step():
        o = dev.forward_train_hip(xs)
        return (o.detach(), *torch.autograd.grad(o, (xs, *params), gs))
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
    for a, b in zip(captured, (out, dx, *(grads[k] for k in PARAMS))):
        assert torch.equal(_bits(a), _bits(b))


# ---- the model -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _net_and_images():
    from vfa_amd.vfanet import VFANet
    torch.manual_seed(21)
    net = VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base="resnet18", mode="3D").train()
    tc.randomise_group_norms(net.base, 22)
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(2, 3, 64, 96, generator=gen)
    x[1] *= 1.5
    cot = tuple(torch.randn(2, c, 64 // s, 96 // s, generator=gen) for c, s in ((128, 8), (256, 16), (512, 32)))
    return net, x, cot


def _trunk_step(net, x, cot):
    """``net.trunk`` forward + backward from the fixed cotangent on a copy -> (maps, {parameter: gradient})."""
    net = copy.deepcopy(net)
    maps = net.trunk(x)
    torch.autograd.backward(maps, [c.to(m) for c, m in zip(cot, maps)])
    return [m.detach() for m in maps], {k: p.grad for k, p in net.base.named_parameters()}


def _counted(monkeypatch, dev):
    """Count the calls of the two block nodes and name the hooked modules (the eight blocks and the stem) that run."""
    from vfa_amd import ops
    calls = {"residual": 0, "projection": 0, "modules": []}

    def counting(name, key):
        real = getattr(ops, name)

        def counted(*args, **kwargs):
            calls[key] += 1
            return real(*args, **kwargs)
        monkeypatch.setattr(ops, name, counted)
    counting("residual_block_train", "residual")
    counting("projection_block_train", "projection")
    blocks = [b for layer in (dev.base.layer1, dev.base.layer2, dev.base.layer3, dev.base.layer4) for b in layer]
    for i, b in enumerate(blocks):
        b.register_forward_hook(lambda *_, name=f"block{i}": calls["modules"].append(name))
    dev.base.conv1.register_forward_hook(lambda *_: calls["modules"].append("stem"))
    return calls


def test_model_with_both_switches_against_the_float64_model(monkeypatch):
    net, x, cot = _net_and_images()
    maps64, grads64 = _trunk_step(copy.deepcopy(net).double(), x.double(), cot)
    maps32, grads32 = _trunk_step(net, x, cot)
    dev = copy.deepcopy(net).to(DEV)
    dev.trunk_convs_train = dev.trunk_proj_train = "hip"
    calls = _counted(monkeypatch, dev)
    maps, grads = _trunk_step(dev, x.to(DEV), cot)
    assert calls["residual"] == 5 and calls["projection"] == 3
    assert calls["modules"] == ["stem"], "only the stem ran as a module"
    assert list(dev.state_dict()) == list(net.state_dict()) and sorted(grads) == sorted(grads64)
    for name, m, m64, m32 in zip(("f8", "f16", "f32"), maps, maps64, maps32):
        cc.check_normwise(m, m64, m32, f"map {name}")
    worst = 0.0
    for k in sorted(grads):
        assert grads[k] is not None, k
        worst = max(worst, cc.check_normwise(grads[k], grads64[k], grads32[k], f"d {k}")[2])
    print(f"model: the worst (N) ratio of a trunk gradient is {worst:.2f} x")


def test_model_with_the_projection_switch_alone(monkeypatch):
    net, x, cot = _net_and_images()
    dev = copy.deepcopy(net).to(DEV)
    dev.trunk_proj_train = "hip"
    calls = _counted(monkeypatch, dev)
    _, grads = _trunk_step(dev, x.to(DEV), cot)
    assert calls["residual"] == 0 and calls["projection"] == 3
    assert sorted(calls["modules"]) == ["block0", "block1", "block3", "block5", "block7", "stem"]
    assert all(v is not None for v in grads.values())


def test_stages_give_the_same_bits_twice_without_the_deterministic_setting():
    assert not torch.are_deterministic_algorithms_enabled()
    net, x, cot = _net_and_images()
    dev = copy.deepcopy(net).to(DEV)
    with torch.no_grad():
        stem = dev.base.stem(x.to(DEV))

    def run():
        trunk = copy.deepcopy(dev.base)
        s = stem.clone().requires_grad_()
        maps = trunk.stages_train_hip(s, identity=True, projection=True)
        torch.autograd.backward(maps, [c.to(DEV) for c in cot])
        return {"stem": s.grad, **{k: p.grad for k, p in trunk.named_parameters() if k.startswith("layer")}}
    first, second = run(), run()
    assert len(first) > 50
    for k in first:
        assert torch.equal(_bits(first[k]), _bits(second[k])), k
