"""Training the trunk's identity residual blocks on the MI355X (``ops.group_norm_stats``, ``ops.group_norm_backward``,
``ops.trunk_conv_weight_grad``, ``ops.trunk_conv_input_grad``, ``ops.residual_block_train``, ``VFANet.trunk_convs_train = "hip"``)
against float64 autograd on the CPU, under the yardsticks of tests/trunk_train_common.py: (N) normwise within 4 x the float32 autograd
chain on the CPU, (E) the derived elementwise bounds.  Shapes are the smallest that can still go wrong: planes of 117 and of 15
positions (fewer than the 32 parts of the statistics), 64 outputs (less than one 128-output tile) on a 5 x 33 map ragged against the
4 x 32 cell tile, 512 channels (two accumulator chains in the input gradient), two images of different scales everywhere.

Asserted in bits: a and b against ``group_norm_affine``, dz, two runs, an image alone against the batch, the block's forward against
``_Block.forward_hip``, frozen weights, the graph replay, and the model with ``"library"`` against ``model.base``.  Every test prints
its measured ratios before it asserts.

Measured on the MI355X: statistics: mean exact, rstd at 0.58 of its bound; GroupNorm backward (N) dy 0.55-0.68 x, dgamma 0.19-0.31 x,
dbeta 0.23-0.49 x; weight gradient (E) at most 1.6 % of the bound, (N) 0.28-0.63 x without and 0.40-0.85 x with the prologue; input
gradient (N) 1.29 x (64 channels) and 2.23 x (512); the blocks: dx 1.22 x and 2.07 x, parameter gradients 0.22-2.24 x; the model: maps
1.29-1.36 x, trunk parameter gradients 0.53-1.98 x."""
import copy
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import conv_common as cc
import conv_grad_common as cg
import trunk_common as tc
import trunk_train_common as tt

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
GROUPS, EPS = 16, 1e-5
U64 = 2.0 ** -53

STATS_SHAPES = [(2, 64, 9, 13), (1, 512, 3, 5)]
GN_SHAPES = STATS_SHAPES + [(2, 128, 8, 32)]
# C = O, L, W; B = 2.  The last: 8 tiles, which slabs_for cuts into 2 slabs at 512 x 512 (5 x 9: 2 tiles in 1 slab)
WGRAD_SHAPES = [(64, 5, 33), (128, 8, 40), (512, 5, 9), (512, 16, 40)]
BLOCK_SHAPES = {64: (2, 64, 12, 40), 512: (2, 512, 3, 5)}


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _gn_case(shape):
    """Inputs on the CPU (never written to) and the forward's a, b, stats and join from the device."""
    from vfa_amd import ops
    B, C, L, W = shape
    y, u, r, gamma, beta = tt.gn_inputs(B, C, L, W, seed=C + L)
    with torch.no_grad():
        a, b, stats = ops.group_norm_stats(y.to(DEV), GROUPS, gamma.to(DEV), beta.to(DEV), EPS)
        out = ops.residual_join(y.to(DEV), (a, b), r.to(DEV))
    return y, u, r, gamma, beta, a, b, stats, out


@pytest.mark.parametrize("shape", STATS_SHAPES)
def test_stats_are_the_affines_bits_and_the_float64_statistics(shape):
    """|mean - mean64| <= 4 N u64 mean|y| and |rstd / rstd64 - 1| <= 4 N u64 (E y^2 + mean^2) / (var + eps) + 4 u64: a float64 sum of N
    terms on each side (the kernel's and numpy's), the variance by E y^2 - mean^2 on both, the square root and the division."""
    from vfa_amd import ops
    B, C, L, W = shape
    y, _, _, gamma, beta, a, b, stats, _ = _gn_case(shape)
    with torch.no_grad():
        a0, b0 = ops.group_norm_affine(y.to(DEV), GROUPS, gamma.to(DEV), beta.to(DEV), EPS)
    assert torch.equal(_bits(a), _bits(a0)) and torch.equal(_bits(b), _bits(b0))
    assert stats.shape == (B, GROUPS, 2) and stats.dtype == torch.float64
    mean64, rstd64 = tt.stats64(y, GROUPS, EPS)
    yg = y.double().reshape(B, GROUPS, -1).numpy()
    n = yg.shape[2]
    got = stats.cpu().numpy()
    mean_ratio = np.abs(got[:, :, 0] - mean64) / (4 * n * U64 * np.abs(yg).mean(2))
    sq = (yg * yg).mean(2)
    rstd_ratio = np.abs(got[:, :, 1] / rstd64 - 1) / (4 * n * U64 * (sq + mean64 ** 2) / (sq - mean64 ** 2 + EPS) + 4 * U64)
    print(f"stats {shape}: mean error / bound = {mean_ratio.max():.3g}, rstd error / bound = {rstd_ratio.max():.3g} (N = {n})")
    assert mean_ratio.max() <= 1 and rstd_ratio.max() <= 1


@pytest.mark.parametrize("mode", ["prologue", "out"])
@pytest.mark.parametrize("shape", GN_SHAPES)
def test_group_norm_backward(shape, mode):
    from vfa_amd import ops
    B, C, L, W = shape
    y, u, r, gamma, beta, a, b, stats, out = _gn_case(shape)

    def run(sel=slice(None)):
        mask_out = out[sel] if mode == "out" else None
        return ops.group_norm_backward(u[sel].to(DEV), y[sel].to(DEV), a[sel], b[sel], gamma.to(DEV), stats[sel], GROUPS, mask_out=mask_out)
    got = run()
    dy, dgamma, dbeta = got[0], got[-2], got[-1]
    if mode == "out":
        mask, shortcut = (out.cpu() > 0).numpy(), r
        assert torch.equal(_bits(got[1].cpu()), _bits(torch.where(out.cpu() > 0, u, torch.zeros_like(u)))), "dz"
    else:
        mask, shortcut = tt.mask_prologue(y, a.cpu(), b.cpu()), None
    assert 0.2 < mask.mean() < 0.8
    what = f"{shape} {mode}"
    tt.check_gn_elementwise(dy, y, u, mask, gamma, GROUPS, EPS, f"{what} dy")
    ref64 = tt.gn_autograd(y, u, gamma, beta, GROUPS, EPS, torch.float64, shortcut)
    ref32 = tt.gn_autograd(y, u, gamma, beta, GROUPS, EPS, torch.float32, shortcut)
    for name, mine, r64, r32 in zip(("dy", "dgamma", "dbeta"), (dy, dgamma, dbeta), ref64, ref32):
        cc.check_normwise(mine, r64, r32, f"{what} {name}")
    for first, second in zip(got, run()):                       # the same bits twice
        assert torch.equal(_bits(first), _bits(second))
    if B > 1:                                                   # image 1 alone: its dy and dz bits from the batch
        alone = run(slice(1, 2))
        assert torch.equal(_bits(alone[0][0]), _bits(dy[1]))
        if mode == "out":
            assert torch.equal(_bits(alone[1][0]), _bits(got[1][1]))
    none = ops.group_norm_backward(u.to(DEV), y.to(DEV), a, b, gamma.to(DEV), stats, GROUPS, mask_out=out if mode == "out" else None,
                                   want_params=False)
    assert none[-1] is None and none[-2] is None and torch.equal(_bits(none[0]), _bits(dy))


@pytest.mark.parametrize("with_affine", [False, True])
@pytest.mark.parametrize("shape", WGRAD_SHAPES)
def test_weight_gradient_with_prologue(shape, with_affine):
    from vfa_amd import ops
    C, L, W = shape
    x, _, g = cg.inputs(2, C, C, L, W, seed=C + L)
    affine = tt.shifted_affine(x, seed=C) if with_affine else None
    if with_affine:
        below = float((tc.prologue32(x, affine) == 0).float().mean())
        print(f"{shape}: {below:.2f} of the values are below zero behind the affine")
        assert 0.4 < below < 0.6
    dev_affine = None if affine is None else tuple(t.to(DEV) for t in affine)
    dw = ops.trunk_conv_weight_grad(g.to(DEV), x.to(DEV), dev_affine)
    assert dw.shape == (C, C, 3, 3) and dw.is_contiguous()
    tt.check_wgrad(dw, g, x, affine, f"{shape} dW{' with the prologue' if with_affine else ''}")
    assert torch.equal(_bits(dw), _bits(ops.trunk_conv_weight_grad(g.to(DEV), x.to(DEV), dev_affine)))
    if not with_affine and C * C <= 256 * 256:                 # the slabs of slabs_for are those of the heads' kernel up to 256 x 256
        assert torch.equal(_bits(dw), _bits(ops.conv3x3_weight_grad(g.to(DEV), x.to(DEV))[0]))
    zero = ops.trunk_conv_weight_grad(torch.zeros_like(g).to(DEV), x.to(DEV), dev_affine)
    assert not zero.any() and not zero.isnan().any()


@pytest.mark.parametrize("C", [64, 512])
def test_input_gradient(C):
    from vfa_amd import ops
    x, w, g = cg.inputs(2, C, C, 5, 33, seed=C + 7)
    dx = ops.trunk_conv_input_grad(g.to(DEV), w.to(DEV))
    assert dx.shape == x.shape and dx.is_contiguous()
    tc.check_elementwise(dx, g, cg.transposed_flipped(w), 1, f"C = {C} dX")
    cc.check_normwise(dx, cg.grads64(x, w, g, 1)[0], cg.grads32(x, w, g, 1)[0], f"C = {C} dX")
    alone = ops.trunk_conv_input_grad(g[1:].to(DEV), w.to(DEV))
    assert torch.equal(_bits(alone[0]), _bits(dx[1]))


# ---- the block -------------------------------------------------------------------------------------------------------------------

PARAMS = ("conv1.weight", "bn1.weight", "bn1.bias", "conv2.weight", "bn2.weight", "bn2.bias")


def _block_step(block, x, g, frozen=False):
    """forward + backward of ``_Block.forward_train_hip`` on fresh leaves of a copy -> (out, dx, {parameter: gradient})."""
    block = copy.deepcopy(block).to(DEV).requires_grad_(not frozen)
    xd = x.to(DEV).requires_grad_()
    out = block.forward_train_hip(xd)
    out.backward(g.to(DEV))
    return out.detach(), xd.grad, {k: p.grad for k, p in block.named_parameters()}


@functools.lru_cache(maxsize=None)
def _block_case(C):
    B, _, L, W = BLOCK_SHAPES[C]
    block = tt.block_of(C, seed=C)
    x = tc.inputs(B, C, C, L, W, seed=C + 3, nonneg=True)[0]
    gen = torch.Generator().manual_seed(C + 4)
    g = torch.randn(B, C, L, W, generator=gen) * (1.0 + torch.arange(B - 1, -1, -1, dtype=torch.float32).view(B, 1, 1, 1) * 3.0)
    return block, x, g, _block_step(block, x, g)


@pytest.mark.parametrize("C", list(BLOCK_SHAPES))
def test_block_against_the_float64_module(C):
    block, x, g, (out, dx, grads) = _block_case(C)
    with torch.no_grad():
        want = copy.deepcopy(block).to(DEV).forward_hip(x.to(DEV))
    assert out.is_contiguous() and torch.equal(_bits(out), _bits(want)), "the forward is forward_hip's"
    out64, dx64, grads64 = tt.block_step(block, x, g, torch.float64)
    out32, dx32, grads32 = tt.block_step(block, x, g, torch.float32)
    assert sorted(grads) == sorted(PARAMS)
    cc.check_normwise(out, out64, out32, f"C = {C} out")
    cc.check_normwise(dx, dx64, dx32, f"C = {C} dx")
    for k in PARAMS:
        cc.check_normwise(grads[k], grads64[k], grads32[k], f"C = {C} d {k}")


@pytest.mark.parametrize("C", list(BLOCK_SHAPES))
def test_block_bits(C):
    """Two runs without torch's deterministic setting, image 0 alone, frozen weights."""
    assert not torch.are_deterministic_algorithms_enabled()
    block, x, g, (out, dx, grads) = _block_case(C)
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
    """Frozen weights: no weight gradient is launched; x without a gradient: the last input gradient is skipped."""
    from vfa_amd import ops
    block, x, g, (_, dx, grads) = _block_case(64)
    with ops.KernelTimer() as kt:
        _block_step(block, x, g, frozen=True)
    torch.cuda.synchronize()
    seen = kt.summary()
    assert "vfa_trunk_conv_wgrad_f32" not in seen and seen["vfa_group_norm_backward_f32"]["launches"] == 2
    dev = copy.deepcopy(block).to(DEV)
    with ops.KernelTimer() as kt:
        dev.forward_train_hip(x.to(DEV)).backward(g.to(DEV))       # x needs no gradient
    torch.cuda.synchronize()
    seen = kt.summary()
    assert seen["vfa_trunk_conv_wgrad_f32"]["launches"] == 2 and seen["vfa_trunk_conv_f32"]["launches"] == 3   # two forward, one backward
    for k, p in dev.named_parameters():
        assert torch.equal(_bits(p.grad), _bits(grads[k])), k


def test_block_graph_replay_equals_the_eager_step():
    """One forward + backward: a single chain on the capture stream, the default queue count."""
    block, x, g, (out, dx, grads) = _block_case(64)
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


def _trunk_step(net, x, cot, direct=False):
    """``net.trunk`` (``direct``: ``net.base``) forward + backward from the fixed cotangent on a copy -> (maps, {parameter: gradient})."""
    net = copy.deepcopy(net)
    maps = net.base(x) if direct else net.trunk(x)
    torch.autograd.backward(maps, [c.to(m) for c, m in zip(cot, maps)])
    return [m.detach() for m in maps], {k: p.grad for k, p in net.base.named_parameters()}, net


def test_model_trunk_trains_against_the_float64_model(monkeypatch):
    from vfa_amd import ops
    net, x, cot = _net_and_images()
    maps64, grads64, _ = _trunk_step(copy.deepcopy(net).double(), x.double(), cot)
    maps32, grads32, _ = _trunk_step(net, x, cot)
    dev = copy.deepcopy(net).to(DEV)
    dev.trunk_convs_train = "hip"
    blocks = [b for layer in (dev.base.layer1, dev.base.layer2, dev.base.layer3, dev.base.layer4) for b in layer]
    calls = {"block": 0, "modules": []}
    real = ops.residual_block_train

    def counted(*args, **kwargs):
        calls["block"] += 1
        return real(*args, **kwargs)
    monkeypatch.setattr(ops, "residual_block_train", counted)

    def hooked(module, name):
        """The deep copy ``_trunk_step`` runs keeps the hooks of the module it was copied from."""
        module.register_forward_hook(lambda *_: calls["modules"].append(name))
    for i, b in enumerate(blocks):
        hooked(b, f"block{i}")
    hooked(dev.base.conv1, "stem")
    maps, grads, _ = _trunk_step(dev, x.to(DEV), cot)
    assert calls["block"] == 5, "the five identity blocks ran residual_block_train"
    assert sorted(calls["modules"]) == ["block2", "block4", "block6", "stem"], "the projection blocks and the stem ran as modules"
    assert list(dev.state_dict()) == list(net.state_dict()) and sorted(grads) == sorted(grads64)
    for name, m, m64, m32 in zip(("f8", "f16", "f32"), maps, maps64, maps32):
        cc.check_normwise(m, m64, m32, f"map {name}")
    worst = 0.0
    for k in sorted(grads):
        assert grads[k] is not None, k
        worst = max(worst, cc.check_normwise(grads[k], grads64[k], grads32[k], f"d {k}")[2])
    print(f"model: the worst (N) ratio of a trunk gradient is {worst:.2f} x")


def test_model_with_library_is_the_trunk_that_never_heard_of_the_switch():
    net, x, cot = _net_and_images()
    dev = copy.deepcopy(net).to(DEV)
    assert dev.trunk_convs_train == "library"
    was = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True, warn_only=True)   # (two calls of the library's convolutions: the same bits only so)
    try:
        _trunk_step(dev, x.to(DEV), cot)
        maps, grads, _ = _trunk_step(dev, x.to(DEV), cot)
        maps_d, grads_d, _ = _trunk_step(dev, x.to(DEV), cot, direct=True)
    finally:
        torch.use_deterministic_algorithms(was)
    for a, b in zip(maps, maps_d):
        assert torch.equal(_bits(a), _bits(b))
    for k in grads:
        assert torch.equal(_bits(grads[k]), _bits(grads_d[k])), k
