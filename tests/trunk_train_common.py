"""What the tests of training the trunk's identity residual blocks share (tests/test_trunk_train_cpu.py, tests/test_trunk_train.py):
the references from torch autograd on the CPU, a float64 numpy restatement of the three-launch GroupNorm backward of
vfa_amd/csrc/vfa_trunk_grad.hip, and the yardsticks.

Forward: z = gamma (y - mean) rstd + beta per (image, group), a ReLU with mask m behind it, u the gradient behind that ReLU.  With
N = (C / groups) L W values in a group:

    S1[b, c] = sum m u                    S2[b, c] = sum m u y
    A[b, g]  = sum_c gamma_c S1           K[b, g]  = rstd sum_c gamma_c (S2 - mean S1)
    dy = p (m u) + q y + r                p = gamma_c rstd      q = -rstd^2 K / N      r = -rstd A / N - q mean
    dgamma[c] = sum_b rstd (S2 - mean S1)                       dbeta[c] = sum_b S1

(N) normwise: the error against float64 autograd on the CPU is at most 4 x that of the float32 autograd chain on the CPU on the same
    inputs (``conv_common.check_normwise``).
(E) elementwise, the project's derived bounds:
    weight gradient   gamma_n (|g| * |x'|), n = n_wgrad(B, L, W), x' = prologue32(x, affine) on both sides (``check_wgrad``);
    input gradient    n_trunk(O, 9) on the transposed, tap-mirrored weight (``trunk_common.check_elementwise``);
    GroupNorm backward  |dy - dy64| <= gamma_4 (|p| |m u| + |q| |y| + |r|): the kernel rounds each of p, q, r once (3 u) and each of its
    two fmaf once, the float64 sums are far below one u, so 4 u on each term is generous -- with the mask taken from the float32
    forward (``mask_prologue``: fmaf(a, y, b) > 0 in float32, or the given map > 0) and everything else in float64.
"""
import copy

import numpy as np
import torch
import torch.nn.functional as F

import conv_common as cc
import conv_grad_common as cg
import trunk_common as tc

N_GN = 4
PARTS = 32          # kParts of vfa_trunk_grad.hip


def gn_inputs(B, C, L, W, seed):
    """A raw map with images of different scales and offsets, an upstream gradient scaled the other way round, a shortcut, and
    GroupNorm parameters away from 1 and 0."""
    gen = torch.Generator().manual_seed(seed)
    y = torch.randn(B, C, L, W, generator=gen) * (1.0 + torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1) * 2.5) + 0.3
    u = torch.randn(B, C, L, W, generator=gen) * 0.01 * (1.0 + torch.arange(B - 1, -1, -1, dtype=torch.float32).view(B, 1, 1, 1) * 7.0)
    r = torch.randn(B, C, L, W, generator=gen)
    gamma = torch.rand(C, generator=gen) + 0.5
    beta = torch.rand(C, generator=gen) * 0.6 - 0.3
    return y, u, r, gamma, beta


def stats64(y, groups, eps):
    """The float64 mean and rstd of each (image, group) -> two (B, groups) arrays."""
    B = y.shape[0]
    yg = y.double().reshape(B, groups, -1).numpy()
    mean = yg.mean(2)
    var = np.maximum((yg * yg).mean(2) - mean * mean, 0.0)
    return mean, 1.0 / np.sqrt(var + eps)


def affine32(y, gamma, beta, groups, eps):
    """``vfa_group_norm_affine_f32`` restated: a = gamma rstd, b = beta - mean a from the float64 statistics, rounded once."""
    gn = torch.nn.GroupNorm(groups, y.shape[1], eps=eps)
    with torch.no_grad():
        gn.weight.copy_(gamma)
        gn.bias.copy_(beta)
    return tc.emulate_gn_affine(y, gn)


def mask_prologue(y, a, b):
    """fmaf(a, y, b) > 0 in float32: the ReLU a convolution applied as it read y."""
    yn = y.numpy().astype(np.float32)
    an, bn = (np.broadcast_to(t.numpy().astype(np.float32)[:, :, None, None], yn.shape) for t in (a, b))
    return cc.fma32(an, yn, bn) > 0


def gn_backward_restated(y, u, mask, gamma, groups, eps, round32=False, variant=None):
    """The three launches of ``vfa_group_norm_backward_f32`` in float64 numpy -> dict(dy, dz, dgamma, dbeta, p, q, r), p, q, r
    broadcast to (B, C, 1, 1).  ``mask``: a boolean array of y's shape.  ``round32``: as the kernel rounds -- p, q, r to float32 once,
    dy = fmaf(p, m u, fmaf(q, y, r)) in float32, dgamma and dbeta to float32 once.  ``variant``: "no_q" drops the q y term; "mask_y"
    takes the mask from y > 0."""
    B, C, L, W = y.shape
    cg_, plane = C // groups, L * W
    yn, un, ga = y.double().numpy(), u.double().numpy(), gamma.double().numpy()
    if variant == "mask_y":
        mask = yn > 0
    mu = np.where(mask, un, 0.0)
    # launch 1: per (image, channel) the 32 parts of the plane, merged in ascending order
    s1, s2 = np.zeros((B, C)), np.zeros((B, C))
    flat_mu, flat_y = mu.reshape(B, C, plane), yn.reshape(B, C, plane)
    for k in range(PARTS):
        part = slice(plane * k // PARTS, plane * (k + 1) // PARTS)      # (an empty part is a zero)
        s1 += flat_mu[:, :, part].sum(2)
        s2 += (flat_mu[:, :, part] * flat_y[:, :, part]).sum(2)
    # launch 2: the coefficients per (image, channel), dgamma and dbeta over the images
    mean, rstd = stats64(y, groups, eps)
    count = float(cg_ * plane)
    A = (ga[None] * s1).reshape(B, groups, cg_).sum(2)
    K = rstd * (ga[None] * (s2 - np.repeat(mean, cg_, 1) * s1)).reshape(B, groups, cg_).sum(2)
    q = -(rstd * rstd) * K / count
    r = -(rstd * A) / count - q * mean
    p = ga[None] * np.repeat(rstd, cg_, 1)
    q, r = np.repeat(q, cg_, 1), np.repeat(r, cg_, 1)
    dgamma = (np.repeat(rstd, cg_, 1) * (s2 - np.repeat(mean, cg_, 1) * s1)).sum(0)
    dbeta = s1.sum(0)
    p, q, r = (t[:, :, None, None] for t in (p, q, r))
    # launch 3: elementwise
    if round32:
        p32, q32, r32 = (np.broadcast_to(t.astype(np.float32), yn.shape) for t in (p, q, r))
        y32 = yn.astype(np.float32)
        inner = np.zeros_like(y32) if variant == "no_q" else cc.fma32(q32, y32, r32)
        dy = cc.fma32(p32, mu.astype(np.float32), inner)
        dgamma, dbeta = dgamma.astype(np.float32), dbeta.astype(np.float32)
    else:
        dy = p * mu + (0.0 if variant == "no_q" else q * yn + r)
    return dict(dy=torch.from_numpy(np.ascontiguousarray(dy)), dz=torch.from_numpy(mu.astype(np.float32)), dgamma=torch.from_numpy(dgamma),
                dbeta=torch.from_numpy(dbeta), p=p, q=q, r=r, mu=mu)


def check_gn_elementwise(dy, y, u, mask, gamma, groups, eps, what=""):
    """(E) of the GroupNorm backward -> the largest ratio error / bound (printed before the assertion)."""
    ref = gn_backward_restated(y, u, mask, gamma, groups, eps)
    err = (torch.as_tensor(dy).double().cpu() - ref["dy"]).abs()
    bound = torch.from_numpy(cc.gamma(N_GN) * (np.abs(ref["p"]) * np.abs(ref["mu"]) + np.abs(ref["q"]) * np.abs(y.double().numpy())
                                               + np.abs(ref["r"])))
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"(E) {what}: max error / bound = {worst:.3g} (n = {N_GN})")
    assert bool((err <= bound).all()), f"(E) {what}: error / bound = {worst:.3g}"
    return worst


def gn_autograd(y, u, gamma, beta, groups, eps, dtype, shortcut=None):
    """Autograd of ``F.relu(F.group_norm(y) [+ shortcut])`` on the CPU in ``dtype`` with the cotangent u -> (dy, dgamma, dbeta, dz |
    None)."""
    y, ga, be = (t.to(dtype).cpu().clone().requires_grad_(True) for t in (y, gamma, beta))
    s = None if shortcut is None else shortcut.to(dtype).cpu().clone().requires_grad_(True)
    z = F.group_norm(y, groups, ga, be, eps)
    F.relu(z if s is None else z + s).backward(u.to(dtype).cpu())
    return y.grad, ga.grad, be.grad, None if s is None else s.grad


def check_wgrad(dw, g, x, affine, what=""):
    """(E) and (N) of the weight gradient with x' = prologue32(x, affine) on both sides of (E) -> the (N) ratio."""
    cg.check_elementwise(dw, g, tc.prologue32(x, affine), 1, what)

    def chain(dtype):
        w = torch.zeros(g.shape[1], x.shape[1], 3, 3, dtype=dtype, requires_grad=True)
        F.conv2d(tc.prologue(x, affine, dtype), w, padding=1).backward(g.to(dtype))
        return w.grad
    return cc.check_normwise(dw, chain(torch.float64), chain(torch.float32), what)[2]


def shifted_affine(x, seed):
    """A per (image, channel) affine whose shift sends about half of a'x + b below zero: b = -a median(x[b, c])."""
    B, C = x.shape[:2]
    a = torch.rand(B, C, generator=torch.Generator().manual_seed(seed)) + 0.5
    return a, -a * x.reshape(B, C, -1).median(2).values


def block_of(C, seed):
    """A seeded identity ``_Block`` with randomised GroupNorm parameters."""
    from vfa_amd.vfanet import _Block
    torch.manual_seed(seed)
    return tc.randomise_group_norms(_Block(C, C), seed + 1)


def block_step(block, x, g, dtype):
    """forward + backward of ``_Block.forward`` on the CPU in ``dtype`` -> (out, dx, {parameter: gradient})."""
    block = copy.deepcopy(block).cpu().to(dtype)
    x = x.to(dtype).cpu().clone().requires_grad_(True)
    out = block(x)
    out.backward(g.to(dtype).cpu())
    return out.detach(), x.grad, {k: p.grad for k, p in block.named_parameters()}
