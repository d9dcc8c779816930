"""What the tests of the stem's training path share (tests/test_stem_train_cpu.py, tests/test_stem_train.py): a numpy restatement of
``vfa_stem_pool_backward_f32`` with two WRONG variants, the float64 and float32 autograd chains of the stem on the CPU, and the
operands of the weight gradient.

Pooling backward.  u is the gradient BEHIND the ReLU: a window credits its winning tap whatever the tap's value, and the ReLU's
mask ``fmaf(a, y, b) > 0`` (applied by the GroupNorm backward) removes the credit of a window whose maximum is 0.  ``check_pool_backward``
asks two things of a u on integer-valued operands, both exact: after the mask it EQUALS float64 autograd of ``max_pool2d(relu(a y + b),
3, 2, 1)``, and before the mask every window has credited exactly one position INSIDE the map, so each plane of u sums to its plane of
gout.  The first catches a wrong tie rule, the second a tap outside the map that wins (its credit is lost; the mask would hide it).

Weight gradient.  (N) of tests/conv_common.py: ||dw - dw64|| / ||dw64|| <= 4 x the same quantity of the float32 autograd chain on the
CPU.  With integer operands whose sums stay below 2^24 the kernel must EQUAL float64.
"""
import copy

import numpy as np
import torch
import torch.nn.functional as F

import conv_common as cc
import stem_common as sc

PARAMS = ("conv1.weight", "bn1.weight", "bn1.bias")
MAX_SLABS = 64      # kMaxSlabs of vfa_stem.h


def slabs(L, W):
    """``wgrad_slabs`` of the (L, W) IMAGE -> (tiles, slabs): tiles of 4 x 32 output cells, at most 64 slabs."""
    Lo, Wo = sc.out_size(L), sc.out_size(W)
    tiles = -(-Lo // sc.TILE[0]) * -(-Wo // sc.TILE[1])
    return tiles, min(tiles, MAX_SLABS)


# ---- the pooling's backward ------------------------------------------------------------------------------------------------------

def _taps(y, affine):
    yn = y.numpy().astype(np.float32)
    a, b = (np.broadcast_to(t.numpy().astype(np.float32)[:, :, None, None], yn.shape) for t in affine)
    t = cc.fma32(a, yn, b)
    return np.where(t < 0, np.float32(0), t)                            # (a NaN stays a NaN)


def emulate_pool_backward(gout, y, affine, last_wins=False, outside_zero=False):
    """``vfa_stem_pool_backward_f32`` restated: the taps max(fmaf(a, y, b), 0) in float32; per window the winner under the forward's rule
    ``t > best or t != t`` scanned over (ty, tx) ascending with the taps outside the map skipped; u = the sum of gout over the windows a
    position won, in ascending (i, j) order from +0, in float32.  Two WRONG variants: ``last_wins`` (``t >= best``: the last of equal
    maxima), ``outside_zero`` (a tap outside the map is a zero that can win; its credit falls outside the map)."""
    t = _taps(y, affine)
    g = gout.numpy().astype(np.float32)
    B, C, L, W = t.shape
    Lo, Wo = sc.out_size(L), sc.out_size(W)
    padded = np.full((B, C, L + 3, W + 3), np.float32(0) if outside_zero else -np.inf, np.float32)
    padded[:, :, 1:1 + L, 1:1 + W] = t
    best = np.full((B, C, Lo, Wo), -np.inf, np.float32)
    code = np.full((B, C, Lo, Wo), -1, np.int64)
    for ty in range(3):
        for tx in range(3):
            tap = padded[:, :, ty:ty + 2 * (Lo - 1) + 1:2, tx:tx + 2 * (Wo - 1) + 1:2]
            wins = ((tap >= best) if last_wins else (tap > best)) | np.isnan(tap)
            best = np.where(wins, tap, best)
            code = np.where(wins, 3 * ty + tx, code)
    u = np.zeros((B, C, L + 3, W + 3), np.float32)
    for ty in (2, 1, 0):            # position p = 2 i - 1 + ty: ascending i is descending ty
        for tx in (2, 1, 0):
            u[:, :, ty:ty + 2 * (Lo - 1) + 1:2, tx:tx + 2 * (Wo - 1) + 1:2] += np.where(code == 3 * ty + tx, g, np.float32(0))
    return torch.from_numpy(np.ascontiguousarray(u[:, :, 1:1 + L, 1:1 + W]))


def pool_backward64(gout, y, affine):
    """float64 autograd of ``max_pool2d(relu(a y + b), 3, 2, 1)`` with respect to ``a y + b``: the ReLU's mask is applied."""
    a, b = (t.double()[:, :, None, None] for t in affine)
    z = (a * y.double() + b).requires_grad_()
    F.max_pool2d(F.relu(z), 3, stride=2, padding=1).backward(gout.double())
    return z.grad


def check_pool_backward(u, gout, y, affine, what=""):
    """The two exact conditions of the module docstring, for integer-valued gout, y, a and b."""
    u = torch.as_tensor(u).double().cpu()
    mask = torch.from_numpy(_taps(y, affine) > 0)
    want = pool_backward64(gout, y, affine)
    wrong = int((u * mask != want).sum())
    print(f"pool backward {what}: {wrong} of {u.numel()} masked elements differ from float64 autograd")
    assert wrong == 0, f"pool backward {what}: {wrong} masked elements differ"
    lost = (u.sum((2, 3)) - gout.double().sum((2, 3))).abs().max()
    print(f"pool backward {what}: the largest difference between a plane's sum of u and of gout is {float(lost):g}")
    assert float(lost) == 0, f"pool backward {what}: a window's credit fell outside the map ({float(lost):g})"


def pool_inputs(B, C, L, W, seed, integer):
    """(gout, y, (a, b)): images of different scales, a and b of both signs.  ``integer``: every value a small integer, y in
    {-2 .. 2} and full of ties, so the taps, the sums and float64 autograd are exact."""
    gen = torch.Generator().manual_seed(seed)
    Lo, Wo = sc.out_size(L), sc.out_size(W)
    if integer:
        y = torch.randint(-2, 3, (B, C, L, W), generator=gen).float()
        a = torch.randint(1, 3, (B, C), generator=gen).float() * (1 - 2 * torch.randint(0, 2, (B, C), generator=gen).float())
        b = torch.randint(-1, 2, (B, C), generator=gen).float()
        gout = torch.randint(-3, 4, (B, C, Lo, Wo), generator=gen).float()
    else:
        y = torch.randn(B, C, L, W, generator=gen) * (1.0 + 2.5 * torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1))
        a, b = torch.randn(B, C, generator=gen), torch.randn(B, C, generator=gen)
        gout = torch.randn(B, C, Lo, Wo, generator=gen)
    if B * C > 1:
        a.view(-1)[0], a.view(-1)[-1] = -a.view(-1)[0].abs(), a.view(-1)[-1].abs()       # both signs whatever the seed
    return gout, y, (a, b)


# ---- the weight gradient -----------------------------------------------------------------------------------------------------------

def wgrad(g, x, dtype):
    """dL/dweight of ``F.conv2d(x, w, stride=2, padding=3)`` by autograd on the CPU in ``dtype`` -> (O, 3, 7, 7)."""
    w = torch.zeros(g.shape[1], 3, 7, 7, dtype=dtype, requires_grad=True)
    F.conv2d(x.to(dtype).cpu(), w, stride=2, padding=3).backward(g.to(dtype).cpu())
    return w.grad


def emulate_wgrad(g, x, pad=3, swap=False):
    """The definition restated in float64 and rounded once: dw[o, c, ky, kx] = sum g[b, o, i, j] x[b, c, 2 i + ky - pad, 2 j + kx - pad].
    Two WRONG variants for the yardstick to catch: ``pad`` other than 3, ``swap`` (ky and kx exchanged on the image side)."""
    gn, xn = g.numpy().astype(np.float64), x.numpy().astype(np.float64)
    B, O, Lo, Wo = gn.shape
    far = 3 + 6
    xp = np.pad(xn, ((0, 0), (0, 0), (far, far + 1), (far, far + 1)))
    dw = np.zeros((O, 3, 7, 7))
    for c in range(3):
        for ky in range(7):
            for kx in range(7):
                ty, tx = (kx, ky) if swap else (ky, kx)
                y0, x0 = far - pad + ty, far - pad + tx
                tap = xp[:, c, y0:y0 + 2 * (Lo - 1) + 1:2, x0:x0 + 2 * (Wo - 1) + 1:2]
                dw[:, c, ky, kx] = np.einsum("boij,bij->o", gn, tap)
    return torch.from_numpy(dw.astype(np.float32))


def wgrad_inputs(B, O, L, W, seed, integer=False):
    """(g, x): ``stem_common.inputs`` (images of different scales) and a gradient of the raw map; ``integer``: values in {-2 .. 2}."""
    gen = torch.Generator().manual_seed(seed + 1000)
    Lo, Wo = sc.out_size(L), sc.out_size(W)
    if integer:
        return (torch.randint(-2, 3, (B, O, Lo, Wo), generator=gen).float(), torch.randint(-2, 3, (B, 3, L, W), generator=gen).float())
    x, _ = sc.inputs(B, O, L, W, seed)
    return torch.randn(B, O, Lo, Wo, generator=gen), x


# ---- the node and the model --------------------------------------------------------------------------------------------------------

def stem_step(trunk, x, g, dtype):
    """forward + backward of the module chain ``_Trunk.stem`` on the CPU in ``dtype`` on a copy -> (out, {parameter: gradient})."""
    t = copy.deepcopy(trunk).cpu().to(dtype)
    out = t.stem(x.to(dtype).cpu())
    out.backward(g.to(dtype).cpu())
    return out.detach(), {k: dict(t.named_parameters())[k].grad for k in PARAMS}


def trunk_step(net, x, cot):
    """``net.trunk`` forward + backward from the fixed cotangent on a copy -> (maps, {parameter: gradient})."""
    net = copy.deepcopy(net)
    maps = net.trunk(x)
    torch.autograd.backward(maps, [c.to(m) for c, m in zip(cot, maps)])
    return [m.detach() for m in maps], {k: p.grad for k, p in net.base.named_parameters()}
