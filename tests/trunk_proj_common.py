"""What the tests of training the trunk's projection blocks share (tests/test_trunk_proj_train_cpu.py, tests/test_trunk_proj_train.py):
the references of the gradients of a stride-2 convolution from torch autograd on the CPU, the yardsticks of
tests/trunk_train_common.py restated for stride 2, and a float64 restatement of ``ops.projection_block_train``.

    y = conv(x, w, stride 2): w (O, C, 3, 3) with padding 1 (kernel 3) or (O, C, 1, 1) without padding (kernel 1); x (B, C, L, W),
    y and its gradient g (B, O, Lo, Wo) with Lo = (L - 1) // 2 + 1.

(N) normwise: at most 4 x the error of the float32 autograd chain on the CPU against float64 autograd (``conv_common.check_normwise``).
(E) elementwise, the bound of ``trunk_train_common.check_wgrad``: |dW - dW64| <= gamma_n (|g| * |x|) with n = ``n_wgrad`` of the cells the
    sum runs over, which at stride 2 are the B Lo Wo cells of g: n = n_wgrad(B, Lo, Wo) -- the same formula, nothing new.
"""
import copy

import numpy as np
import torch
import torch.nn.functional as F

import conv_common as cc
import conv_grad_common as cg
import trunk_common as tc
import trunk_train_common as tt

# (B, C, O, L, W) of x: what each exercises is said in tests/test_trunk_proj_train.py
SHAPES = [(2, 64, 128, 9, 13), (1, 64, 128, 8, 13), (1, 256, 512, 6, 10), (2, 128, 256, 16, 66), (1, 64, 128, 1, 1), (1, 64, 128, 2, 2)]


def down(n):
    return (n - 1) // 2 + 1


def conv_down(x, w):
    return F.conv2d(x, w, stride=2, padding=w.shape[-1] // 2)


def grads(x, w, g, dtype):
    """(dx, dw) of ``conv_down`` from autograd on the CPU in ``dtype``."""
    x, w = x.to(dtype).cpu().clone().requires_grad_(True), w.to(dtype).cpu().clone().requires_grad_(True)
    conv_down(x, w).backward(g.to(dtype).cpu())
    return x.grad, w.grad


def wgrad(g, x, kernel, dtype):
    return grads(x, torch.zeros(g.shape[1], x.shape[1], kernel, kernel), g, dtype)[1]


def inputs(B, C, O, L, W, seed, kernel=3):
    """x and w of ``trunk_common.inputs`` (images of different scales, x an activated map) and an output gradient of the stride-2 size
    whose images are scaled the other way round."""
    x, w = tc.inputs(B, C, O, L, W, seed, k=kernel, nonneg=True)
    gen = torch.Generator().manual_seed(seed + 1000)
    g = torch.randn(B, O, down(L), down(W), generator=gen) * 0.01
    return x, w, g * (1.0 + torch.arange(B - 1, -1, -1, dtype=torch.float32).view(B, 1, 1, 1) * 7.0)


def integer_inputs(B, C, O, L, W, seed, kernel=3):
    """Integer-valued x, w and g with |v| <= 4, each holding a 4 somewhere in every image (so every scale is the same power of two)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randint(-4, 5, (B, C, L, W), generator=gen).float()
    w = torch.randint(-4, 5, (O, C, kernel, kernel), generator=gen).float()
    g = torch.randint(-4, 5, (B, O, down(L), down(W)), generator=gen).float()
    x[:, 0, 0, 0], g[:, 0, 0, 0], w[0, 0, 0, 0] = 4.0, -4.0, 4.0
    return x, w, g


def check_wgrad(dw, g, x, kernel, what=""):
    """(E) and (N) of the stride-2 weight gradient -> the (N) ratio."""
    B, _, Lo, Wo = g.shape
    n = cg.n_wgrad(B, Lo, Wo)
    err = (torch.as_tensor(dw).double().cpu() - wgrad(g, x, kernel, torch.float64)).abs()
    bound = cc.gamma(n) * wgrad(g.abs(), x.abs(), kernel, torch.float64)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"(E) {what}: max error / bound = {worst:.3g} (n = {n})")
    assert bool((err <= bound).all()), f"(E) {what}: error / bound = {worst:.3g}"
    return cc.check_normwise(dw, wgrad(g, x, kernel, torch.float64), wgrad(g, x, kernel, torch.float32), what)[2]


# ---- the block ---------------------------------------------------------------------------------------------------------------------

PARAMS = ("conv1.weight", "bn1.weight", "bn1.bias", "conv2.weight", "bn2.weight", "bn2.bias", "downsample.0.weight", "downsample.1.weight",
          "downsample.1.bias")


def block_of(cin, cout, seed):
    """A seeded projection ``_Block`` with randomised GroupNorm parameters."""
    from vfa_amd.vfanet import _Block
    torch.manual_seed(seed)
    return tc.randomise_group_norms(_Block(cin, cout, 2), seed + 1)


def block_inputs(block, B, L, W, seed):
    cin, cout = block.conv1.in_channels, block.conv1.out_channels
    x = tc.inputs(B, cin, cout, L, W, seed=seed, nonneg=True)[0]
    gen = torch.Generator().manual_seed(seed + 1)
    g = torch.randn(B, cout, down(L), down(W), generator=gen) * (1.0 + torch.arange(B - 1, -1, -1, dtype=torch.float32).view(B, 1, 1, 1) * 3.0)
    return x, g


def block_restated(block, x, g):
    """``ops.projection_block_train`` in float64 on the CPU, step by step as the node does it -- the masks from the float64 forward,
    the GroupNorm backward of ``trunk_train_common.gn_backward_restated``, the convolution gradients of ``torch.nn.grad`` ->
    (out, dx, {parameter: gradient})."""
    b = copy.deepcopy(block).cpu().double()
    x, g = x.double().cpu(), g.double().cpu()
    groups, eps = b.bn1.num_groups, b.bn1.eps
    w1, w2, wd = b.conv1.weight.detach(), b.conv2.weight.detach(), b.downsample[0].weight.detach()
    g1, g2, gd = b.bn1.weight.detach(), b.bn2.weight.detach(), b.downsample[1].weight.detach()
    with torch.no_grad():
        y1 = conv_down(x, w1)
        z1 = F.relu(b.bn1(y1))
        y2 = F.conv2d(z1, w2, padding=1)
        yd = conv_down(x, wd)
        out = F.relu(b.bn2(y2) + b.downsample[1](yd))
    mask = (out > 0).numpy()
    r2 = tt.gn_backward_restated(y2, g, mask, g2, groups, eps)
    dz = torch.from_numpy(r2["mu"])
    rd = tt.gn_backward_restated(yd, dz, mask, gd, groups, eps)        # u = dz behind the same mask
    dy2, dyd = r2["dy"], rd["dy"]
    dw2 = torch.nn.grad.conv2d_weight(z1, w2.shape, dy2, padding=1)
    dx1 = torch.nn.grad.conv2d_input(z1.shape, w2, dy2, padding=1)
    r1 = tt.gn_backward_restated(y1, dx1, (z1 > 0).numpy(), g1, groups, eps)
    dy1 = r1["dy"]
    dw1 = torch.nn.grad.conv2d_weight(x, w1.shape, dy1, stride=2, padding=1)
    dwd = torch.nn.grad.conv2d_weight(x, wd.shape, dyd, stride=2)
    dx = torch.nn.grad.conv2d_input(x.shape, w1, dy1, stride=2, padding=1) + torch.nn.grad.conv2d_input(x.shape, wd, dyd, stride=2)
    return out, dx, {"conv1.weight": dw1, "bn1.weight": r1["dgamma"], "bn1.bias": r1["dbeta"], "conv2.weight": dw2, "bn2.weight": r2["dgamma"],
                     "bn2.bias": r2["dbeta"], "downsample.0.weight": dwd, "downsample.1.weight": rd["dgamma"], "downsample.1.bias": rd["dbeta"]}
