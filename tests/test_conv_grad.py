"""Training the dense 3x3 convolution on the MI355X (``ops.conv3x3_train``, ``ops.conv3x3_input_grad``, ``ops.conv3x3_weight_grad``,
``VFANet.head_convs_train = "hip"``) against float64 autograd of ``F.conv2d`` / of the module chain on the CPU, under the two
yardsticks of tests/conv_grad_common.py: (E) elementwise with n = 3 B L W + 8 + B slabs (weight), 27 O + 12 (input: the forward
kernel over O channels) and 2 (bias), (N) normwise within 4 x the float32 autograd chain on the CPU.  Shapes are the smallest that
can still go wrong: A a map ragged against the 4 x 32 cell tile in both directions with O = 96 ragged against the 128-output tile and
two chunks of inputs (6 slabs of one tile); B a map smaller than the dilation's reach (one slab); C the model's 256 x 256 widths on
20 x 24 cells, 5 tiles and so 5 slabs, with dilation 1 and 2; one case with x channels-last and g a slice of a larger tensor.

The weight gradient is NOT asserted bit-equal to ``emulate_wgrad``: the order in which a v_mfma_f32_32x32x16_f16 adds its 16
products and the accumulator is not documented, and the restatement rounds once per product and step (the forward kernel's tests
make the same choice).  What is asserted in bits is everything the kernels define themselves: two runs, a frame alone against the
batch, every layout, the graph replay, and the merge -- the float32 partials the kernel wrote, added in float64 in ascending
(frame, slab) order and rounded once on the CPU, are the bits of dW.

Measured on the MI355X (each test prints its own before it asserts): (E) at most 5 % of the bound (shape B; 0.03 % at 256 x 256);
(N) dW 0.22-1.46 x (1.4e-7 at 256 x 256 against the CPU's 6e-7; the numpy restatement gives 1.15e-7 where the kernel gives 1.42e-7
on shape A), dX 1.1-2.3 x, db 0.03-0.5 x; the model's outputs 2.0-2.4 x, its parameter gradients 0.3-3.7 x (the largest:
fuse.1.bias), d topdown 2.1 x.  (A convolution's bias in front of a training-mode BatchNorm has a gradient that is zero in exact
arithmetic: there (N) compares two rounding noises, the kernel's float64 bias sums against the CPU's float32 ones, 0.3 x.)"""
import copy
import functools
from types import SimpleNamespace

import pytest
import torch

import conv_common as cc
import conv_grad_common as cg

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

CASES = {  # name: (B, C, O, L, W, dilation, x layout, g layout)
    "A": (2, 64, 96, 9, 37, 1, "nchw", "nchw"),
    "B": (2, 32, 32, 3, 5, 4, "nchw", "nchw"),
    "C_d1": (2, 256, 256, 20, 24, 1, "nchw", "nchw"),
    "C_d2": (2, 256, 256, 20, 24, 2, "nchw", "nchw"),
    "A_strided": (2, 64, 96, 9, 37, 1, "nhwc", "slice"),
}


def _bits(t):
    return t.contiguous().view(torch.int32)


def _layout(x, layout):
    """The same values as NCHW, channels-last, or a non-contiguous slice of a larger tensor, on the device."""
    x = x.to(DEV)
    if layout == "nchw":
        return x.contiguous()
    if layout == "nhwc":
        return x.contiguous(memory_format=torch.channels_last)
    B, C, L, W = x.shape
    big = torch.full((B + 1, C + 8, L + 2, W + 3), 7.0, device=DEV)
    big[1:, 4:4 + C, 1:1 + L, 2:2 + W] = x
    view = big[1:, 4:4 + C, 1:1 + L, 2:2 + W]
    assert not view.is_contiguous()
    return view


def _step(x, w, bias, g, d, x_layout="nchw", g_layout="nchw", needs=(True, True, True)):
    """One forward + backward of ``ops.conv3x3_train`` on fresh leaves -> (y, dX, dW, db)."""
    from vfa_amd import ops
    xd = _layout(x, x_layout).detach().requires_grad_(needs[0])
    wd = w.to(DEV).requires_grad_(needs[1])
    bd = bias.to(DEV).requires_grad_(needs[2])
    y = ops.conv3x3_train(xd, wd, bd, d)
    y.backward(_layout(g, g_layout))
    return y.detach(), xd.grad, wd.grad, bd.grad


@functools.lru_cache(maxsize=None)
def _case(name):
    """Inputs, the CPU references (computed once, never written to) and the kernels' gradients."""
    B, C, O, L, W, d, x_layout, g_layout = CASES[name]
    x, w, g = cg.inputs(B, C, O, L, W, seed=C + O + L + d)   # (A and A_strided: the same values)
    bias = torch.randn(O, generator=torch.Generator().manual_seed(3)) * 0.1
    return x, w, bias, g, d, cg.grads64(x, w, g, d, bias), cg.grads32(x, w, g, d, bias), _step(x, w, bias, g, d, x_layout, g_layout)


@pytest.mark.parametrize("name", list(CASES))
def test_gradients_against_float64_autograd(name):
    x, w, bias, g, d, (dx64, dw64, db64), (dx32, dw32, db32), (y, dx, dw, db) = _case(name)
    assert dx.shape == x.shape and dw.shape == w.shape and db.shape == bias.shape and dw.is_contiguous()
    cg.check_elementwise(dw, g, x, d, f"{name} dW")
    cg.check_normwise(dw, dw64, dw32, f"{name} dW")
    cc.check_elementwise(dx, g, cg.transposed_flipped(w), d, cc.n_dense(w.shape[0]), f"{name} dX")
    cg.check_normwise(dx, dx64, dx32, f"{name} dX")
    cg.check_bias_elementwise(db, g, f"{name} db")
    cg.check_normwise(db, db64, db32, f"{name} db")
    restated = cg.normwise(cg.emulate_wgrad(g, x, d), dw64) if x.shape[1] <= 64 else float("nan")
    print(f"{name} dW: kernel {cg.normwise(dw, dw64):.3g}, restatement {restated:.3g} (not asserted equal: see the module's docstring)")


@pytest.mark.parametrize("name", ["A", "A_strided", "C_d2"])
def test_forward_is_the_inference_kernels_bits(name):
    from vfa_amd import ops
    x, w, bias, g, d, _, _, (y, _, _, _) = _case(name)
    with torch.no_grad():
        want = ops.conv3x3(x.to(DEV), w.to(DEV), d, shift=bias.to(DEV))
    assert y.shape == want.shape and y.is_contiguous() and torch.equal(_bits(y), _bits(want))


@pytest.mark.parametrize("name", ["A", "C_d1"])
def test_the_same_step_twice_gives_the_same_bits_without_deterministic_mode(name):
    assert not torch.are_deterministic_algorithms_enabled()
    x, w, bias, g, d, _, _, first = _case(name)
    again = _step(x, w, bias, g, d)
    for what, a, b in zip(("y", "dX", "dW", "db"), first, again):
        assert torch.equal(_bits(a), _bits(b)), what
    assert float(first[2].abs().max()) > 0


def test_every_layout_gives_the_same_bits():
    """x channels-last and g a slice of a larger tensor: read through their strides, the bits of the contiguous call."""
    from vfa_amd import ops
    for a, b in zip(_case("A")[7], _case("A_strided")[7]):
        assert torch.equal(_bits(a), _bits(b))
    x, w, bias, g, d = _case("A")[:5]
    gv, xv = _layout(g, "slice"), _layout(x, "nhwc")
    assert not gv.is_contiguous() and xv.stride(1) == 1
    dw, db = ops.conv3x3_weight_grad(gv, xv, d, want_bias=True)     # (the wrappers themselves: autograd passes no other tensor)
    assert torch.equal(_bits(dw), _bits(_case("A")[7][2])) and torch.equal(_bits(db), _bits(_case("A")[7][3]))
    assert torch.equal(_bits(ops.conv3x3_input_grad(_layout(g, "nhwc"), w.to(DEV), d)), _bits(_case("A")[7][1]))


@pytest.mark.parametrize("name", ["A", "C_d2"])
def test_batch_is_the_fixed_order_merge_of_the_frames(name):
    from vfa_amd import ops
    x, w, bias, g, d, _, _, (_, dx, dw, db) = _case(name)
    B, _, L, W = x.shape
    gd, xd = g.to(DEV), x.to(DEV)
    dw_again, _, partials = ops.conv3x3_weight_grad(gd, xd, d, want_partials=True)
    assert partials.shape == (B, cg.slabs(L, W), 9, w.shape[0], w.shape[1]) and cg.slabs(L, W) >= 2
    partials = partials.cpu()
    for b in range(B):
        alone = _step(x[b:b + 1], w, bias, g[b:b + 1], d)
        assert torch.equal(_bits(alone[1][0]), _bits(dx[b])), f"dX of frame {b} alone"
        one = ops.conv3x3_weight_grad(gd[b:b + 1], xd[b:b + 1], d, want_partials=True)[2].cpu()
        assert torch.equal(_bits(one[0]), _bits(partials[b])), f"partials of frame {b} alone"
    total = torch.zeros(partials.shape[2:], dtype=torch.float64)
    for b in range(B):
        for s in range(partials.shape[1]):                     # ascending (frame, slab), float64, one rounding
            total = total + partials[b, s].double()
    merged = total.float().permute(1, 2, 0).reshape(w.shape)
    assert torch.equal(_bits(merged), _bits(dw.cpu())) and torch.equal(_bits(dw_again), _bits(dw))


def test_only_the_gradients_that_are_needed_and_the_same_bits():
    x, w, bias, g, d, _, _, (_, dx, dw, db) = _case("A")
    _, dx1, dw1, db1 = _step(x, w, bias, g, d, needs=(True, False, False))
    assert dw1 is None and db1 is None and torch.equal(_bits(dx1), _bits(dx))
    _, dx2, dw2, db2 = _step(x, w, bias, g, d, needs=(False, True, False))
    assert dx2 is None and db2 is None and torch.equal(_bits(dw2), _bits(dw))
    _, dx3, dw3, db3 = _step(x, w, bias, g, d, needs=(False, False, True))
    assert dx3 is None and dw3 is None and torch.equal(_bits(db3), _bits(db))


def test_zero_gradient_gives_exact_zeros():
    x, w, bias, g, d = _case("A")[:5]
    _, dx, dw, db = _step(x, w, bias, torch.zeros_like(g), d)
    for t in (dx, dw, db):
        assert not t.isnan().any() and not t.any()
    half = g.clone()
    half[0] = 0                                                  # one frame's absmax is zero, the other's is not
    _, dx, dw, db = _step(x, w, bias, half, d)
    assert not dx[0].any() and dx[1].any() and not dw.isnan().any()
    assert torch.equal(_bits(dw), _bits(_step(x[1:], w, bias, g[1:], d)[2]))   # (a zero partial added in float64 changes nothing)


def test_second_backward_raises():
    from vfa_amd import ops
    x, w, bias, g, d = _case("B")[:5]
    xd, wd = x.to(DEV).requires_grad_(), w.to(DEV).requires_grad_()
    y = ops.conv3x3_train(xd, wd, None, d)
    (dx,) = torch.autograd.grad((y * y).sum(), xd, create_graph=True)   # (the incoming gradient 2 y carries a graph)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        dx.sum().backward()
    with pytest.raises(ValueError, match="multiples of 32"):
        ops.conv3x3_train(x.to(DEV), torch.zeros(40, 32, 3, 3, device=DEV).requires_grad_())
    with pytest.raises(ValueError, match="dilation"):
        ops.conv3x3_train(xd, wd, None, 5)


def test_graph_replay_equals_the_eager_step():
    """One forward + backward: a single chain on the capture stream, the default queue count."""
    from vfa_amd import ops
    x, w, bias, g, d, _, _, eager_first = _case("A")
    x2, g2 = x.flip(3) * 1.5, g.flip(2) * 0.5
    eager_second = _step(x2, w, bias, g2, d)
    xs, gs = x.to(DEV).requires_grad_(), g.to(DEV).clone()
    ws, bs = w.to(DEV).requires_grad_(), bias.to(DEV).requires_grad_()

    def step():
        y = ops.conv3x3_train(xs, ws, bs, d)
        return (y.detach(), *torch.autograd.grad(y, (xs, ws, bs), gs))
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
    for a, b in zip(captured, eager_first):
        assert torch.equal(_bits(a), _bits(b))
    with torch.no_grad():
        xs.copy_(x2)
        gs.copy_(g2)
    graph.replay()
    for a, b in zip(captured, eager_second):
        assert torch.equal(_bits(a), _bits(b))
    assert not torch.equal(_bits(eager_first[2]), _bits(eager_second[2]))


# ---- the model -------------------------------------------------------------------------------------------------------------------

CONVERTED = ("fuse.0", "fuse.3", "tytx_pred.0", "thtwtl_pred.0")


@functools.lru_cache(maxsize=None)
def _net_and_topdown():
    from vfa_amd.vfanet import VFANet
    torch.manual_seed(15)
    net = VFANet(SimpleNamespace(data="MultiviewC", image_size=(720, 1280)), base="resnet18", mode="3D").train()
    gen = torch.Generator().manual_seed(17)
    topdown = torch.randn(2, 256, 12, 40, generator=gen)
    topdown[1] *= 2.5
    coef = {k: torch.randn(s, generator=gen) for k, s in
            (("heatmap", (2, 1, 12, 40)), ("loc_offset", (2, 12, 40, 2)), ("dim_offset", (2, 12, 40, 3)), ("rotation", (2, 12, 40, 360)))}
    return net, topdown, coef


def _model_step(net, topdown, coef, direct=False):
    """heads forward + backward from a scalar loss over all outputs on a copy of ``net`` (training-mode BatchNorm moves the running
    statistics) -> (outputs, {parameter: gradient}, d topdown).  ``direct``: the heads written out on the modules, by a caller that
    never heard of the switches."""
    net = copy.deepcopy(net)
    topdown = topdown.detach().clone().requires_grad_()
    if direct:
        fused = net.fuse(topdown)
        out = {"heatmap": net.map_classifier(fused), "loc_offset": net.tytx_pred(topdown).permute(0, 2, 3, 1),
               "dim_offset": net.thtwtl_pred(topdown).permute(0, 2, 3, 1), "rotation": net.orient_pred(fused).permute(0, 2, 3, 1)}
    else:
        out = net.heads(topdown)
    sum((out[k] * coef[k].to(out[k])).sum() for k in sorted(out)).backward()
    grads = {k: p.grad for k, p in net.named_parameters() if p.grad is not None}
    return {k: v.detach() for k, v in out.items()}, grads, topdown.grad


def test_model_heads_train_against_the_float64_modules():
    net, topdown, coef = _net_and_topdown()
    out64, grads64, dt64 = _model_step(copy.deepcopy(net).double(), topdown.double(), coef)
    out32, grads32, dt32 = _model_step(net, topdown, coef)
    dev = copy.deepcopy(net).to(DEV)
    dev.head_convs_train = "hip"
    assert not torch.are_deterministic_algorithms_enabled()
    out, grads, dt = _model_step(dev, topdown.to(DEV), coef)
    out_again, grads_again, dt_again = _model_step(dev, topdown.to(DEV), coef)
    assert sorted(grads) == sorted(grads64) and all(any(k.startswith(c) for k in grads) for c in CONVERTED)
    assert list(dev.state_dict()) == list(net.state_dict())
    for k in sorted(out):
        cc.check_normwise(out[k], out64[k], out32[k], f"output {k}")
    worst = 0.0
    for k in sorted(grads):
        worst = max(worst, cc.check_normwise(grads[k], grads64[k], grads32[k], f"d {k}")[2])
    worst = max(worst, cc.check_normwise(dt, dt64, dt32, "d topdown")[2])
    print(f"model: the worst (N) ratio of a gradient is {worst:.2f} x")
    for c in CONVERTED:                                         # the same step twice: the same bits where the HIP kernels made them
        assert torch.equal(_bits(grads[c + ".weight"]), _bits(grads_again[c + ".weight"])), c


def test_model_with_library_is_the_model_that_never_heard_of_the_switch():
    net, topdown, coef = _net_and_topdown()
    dev = copy.deepcopy(net).to(DEV)
    assert dev.head_convs_train == "library"
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)   # (two calls of the library's convolutions: the same bits only so)
    try:
        _model_step(dev, topdown.to(DEV), coef)
        out, grads, dt = _model_step(dev, topdown.to(DEV), coef)
        out_d, grads_d, dt_d = _model_step(dev, topdown.to(DEV), coef, direct=True)
    finally:
        torch.use_deterministic_algorithms(was)
    assert sorted(out) == sorted(out_d) and sorted(grads) == sorted(grads_d)
    for k in out:
        assert torch.equal(_bits(out[k]), _bits(out_d[k])), k
    for k in grads:
        assert torch.equal(_bits(grads[k]), _bits(grads_d[k])), k
    assert torch.equal(_bits(dt), _bits(dt_d))
