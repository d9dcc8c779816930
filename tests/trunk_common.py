"""What the tests of the trunk's convolutions share (tests/test_trunk_convs_cpu.py, tests/test_trunk_convs.py): the yardsticks of
tests/conv_common.py with a stride, a 1 x 1 weight and the prologue, and a numpy restatement of the arithmetic of
vfa_amd/csrc/vfa_trunk.hip (the dense kernel of vfa_dense.h) -- the convolution, the GroupNorm affine, the join, a block and the whole trunk.

(E) elementwise:  |y - y64| <= gamma_n (|x'| conv |w|),  n = 27 C + 12 with nine taps and 3 C + 12 with one: three products of
    taps x C terms in any order, the split residuals, the dropped lo.lo, the scaling.  x' is the FLOAT32 result of the prologue
    max(fmaf(a, x, b), 0) (``prologue32``), so both sides see the same operand.
(N) normwise:  ||y - y64|| / ||y64|| <= 4 x the same quantity of the float32 library chain on the CPU, on the same inputs.
"""
import copy

import numpy as np
import torch
import torch.nn.functional as F

import conv_common as cc

SPLIT_C = 256       # kSplitC of vfa_conv.h


def n_trunk(C, taps):
    return 3 * taps * C + 12


def out_size(n, s):
    return (n - 1) // s + 1


def conv(x, w, stride, dtype):
    return F.conv2d(x.to(dtype).cpu(), w.to(dtype).cpu(), stride=stride, padding=w.shape[-1] // 2)


def prologue32(x, affine):
    """max(fmaf(a, x, b), 0) in float32, one rounding -> a float32 tensor (x itself without an affine)."""
    if affine is None:
        return x
    a, b = (t.numpy().astype(np.float32)[:, :, None, None] for t in affine)
    xn = x.numpy().astype(np.float32)
    t = cc.fma32(np.broadcast_to(a, xn.shape), xn, np.broadcast_to(b, xn.shape))
    return torch.from_numpy(np.where(t < 0, np.float32(0), t))      # (a NaN stays a NaN, as in the kernel)


def prologue(x, affine, dtype):
    """The library's chain relu(a x + b) in ``dtype``."""
    if affine is None:
        return x.to(dtype)
    return torch.relu(affine[0].to(dtype)[:, :, None, None] * x.to(dtype) + affine[1].to(dtype)[:, :, None, None])


def check_elementwise(y, xp, w, stride, what=""):
    """(E) on the float32 operand ``xp = prologue32(x, affine)`` -> the largest ratio error / bound (printed before the assertion)."""
    n = n_trunk(w.shape[1], w.shape[2] * w.shape[3])
    y = torch.as_tensor(y).double().cpu()
    err = (y - conv(xp, w, stride, torch.float64)).abs()
    bound = cc.gamma(n) * conv(xp.abs(), w.abs(), stride, torch.float64)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"(E) {what}: max error / bound = {worst:.3g} (n = {n})")
    assert bool((err <= bound).all()), f"(E) {what}: error / bound = {worst:.3g}"
    return worst


def check_both(y, x, w, stride, affine=None, what=""):
    """(E) and (N) of a raw convolution with an optional prologue -> the (N) ratio."""
    check_elementwise(y, prologue32(x, affine), w, stride, what)
    y64 = conv(prologue(x, affine, torch.float64), w, stride, torch.float64)
    y32 = conv(prologue(x, affine, torch.float32), w, stride, torch.float32)
    return cc.check_normwise(y, y64, y32, what)[2]


def inputs(B, C, O, L, W, seed, k=3, nonneg=False):
    """``cc.inputs`` (images of different scales) with a k x k weight; ``nonneg``: an activated map, as the trunk's convolutions read."""
    x, w = cc.inputs(B, C, O, L, W, seed)
    if k == 1:
        w = w[:, :, 1:2, 1:2].contiguous() * 3.0
    return (x.abs() if nonneg else x), w


def affine_of(B, C, seed, positive_shift=False):
    gen = torch.Generator().manual_seed(seed)
    a = torch.rand(B, C, generator=gen) + 0.5
    b = torch.rand(B, C, generator=gen) + 0.25 if positive_shift else torch.randn(B, C, generator=gen)
    return a, b


def emulate_conv(x, w, stride=1, affine=None, drop_lo=False):
    """The trunk kernel's arithmetic: the prologue in float32, per-image and per-weight power-of-two scales (the image's from the
    finite values the products see: after the prologue, and with one tap at the strided positions), the two-piece fp16 split, per
    16 k the three products x_hi w_lo, x_hi w_hi, x_lo w_hi each added to a float32 accumulator, chunks of 32 channels, taps inside a
    chunk; with C > 256 the chunks of the first half in one chain, the rest in a second, first + second -> float32 (B, O, Lo, Wo).
    ``drop_lo``: the hi pieces alone."""
    xn, wn = prologue32(x, affine).numpy().astype(np.float32), w.numpy().astype(np.float32)
    B, C, L, W = xn.shape
    O, k = wn.shape[0], wn.shape[2]
    pad = k // 2
    Lo, Wo = out_size(L, stride), out_size(W, stride)
    ew = cc.split_exponent(np.abs(wn).max())
    wh, wl = cc.split(wn * np.float32(2.0 ** ew))
    n_chunks = C // cc.CHUNK
    n_first = (n_chunks + 1) // 2 if C > SPLIT_C else n_chunks
    out = np.zeros((B, O, Lo, Wo), np.float32)
    for b in range(B):
        seen = xn[b] if k == 3 else xn[b][:, ::stride, ::stride]
        finite = np.abs(seen[np.isfinite(seen)])
        ea = cc.split_exponent(finite.max() if finite.size else 0.0)
        xh, xl = cc.split(xn[b] * np.float32(2.0 ** ea))
        xh, xl = (np.pad(p, ((0, 0), (pad, pad), (pad, pad))) for p in (xh, xl))
        chains = []
        for chunks in (range(0, n_first), range(n_first, n_chunks)):
            acc = np.zeros((O, Lo, Wo), np.float32)
            for ch in chunks:
                for t in range(k * k):
                    ty, tx = divmod(t, k)
                    for s in range(0, cc.CHUNK, cc.STEP):
                        c = slice(ch * cc.CHUNK + s, ch * cc.CHUNK + s + cc.STEP)
                        ah, al = (p[c, ty:ty + stride * (Lo - 1) + 1:stride, tx:tx + stride * (Wo - 1) + 1:stride] for p in (xh, xl))
                        products = [(wh, ah)] if drop_lo else [(wl, ah), (wh, ah), (wh, al)]
                        for wp, ap in products:
                            acc = (acc.astype(np.float64) + np.einsum("oc,clw->olw", wp[:, c, ty, tx], ap)).astype(np.float32)
            chains.append(acc)
        total = chains[0] + chains[1] if n_first < n_chunks else chains[0]
        out[b] = total * np.float32(2.0 ** -(ea + ew))
    return torch.from_numpy(out)


def emulate_gn_affine(y, gn):
    """``vfa_group_norm_affine_f32``: the statistics in float64, a = gamma rstd and b = beta - mean a rounded once to float32."""
    B, C = y.shape[:2]
    G = gn.num_groups
    yg = y.double().reshape(B, G, -1)
    mean, var = yg.mean(2), yg.var(2, unbiased=False)
    rstd = (1.0 / torch.sqrt(var + gn.eps)).repeat_interleave(C // G, 1)
    ga, be = gn.weight.detach().double()[None], gn.bias.detach().double()[None]
    return (ga * rstd).float(), (be - mean.repeat_interleave(C // G, 1) * ga * rstd).float()


def emulate_join(y, affine, r, r_affine=None):
    """``vfa_residual_join_f32``: max(fmaf(a, y, b) + (r | fmaf(ra, r, rb)), 0), one float32 rounding per operation."""
    def fma(t, ab):
        tn = t.numpy().astype(np.float32)
        a, b = (np.broadcast_to(v.numpy().astype(np.float32)[:, :, None, None], tn.shape) for v in ab)
        return cc.fma32(a, tn, b)
    shortcut = r.numpy().astype(np.float32) if r_affine is None else fma(r, r_affine)
    val = fma(y, affine) + shortcut
    return torch.from_numpy(np.where(val < 0, np.float32(0), val).astype(np.float32))


def emulate_block(block, x):
    """``_Block.forward_hip`` restated."""
    stride = block.conv1.stride[0]
    y1 = emulate_conv(x, block.conv1.weight.detach(), stride)
    y2 = emulate_conv(y1, block.conv2.weight.detach(), 1, emulate_gn_affine(y1, block.bn1))
    if block.downsample is None:
        return emulate_join(y2, emulate_gn_affine(y2, block.bn2), x)
    yd = emulate_conv(x, block.downsample[0].weight.detach(), stride)
    return emulate_join(y2, emulate_gn_affine(y2, block.bn2), yd, emulate_gn_affine(yd, block.downsample[1]))


def emulate_trunk(trunk, x):
    """``_Trunk.forward_hip`` restated: the stem as the float32 library runs it, the residual stages block by block."""
    with torch.no_grad():
        x = F.max_pool2d(F.relu(trunk.bn1(trunk.conv1(x))), 3, stride=2, padding=1)
        maps = []
        for layer in (trunk.layer1, trunk.layer2, trunk.layer3, trunk.layer4):
            for block in layer:
                x = emulate_block(block, x)
            maps.append(x)
    return maps[1], maps[2], maps[3]


def randomise_group_norms(module, seed):
    """GroupNorm weights in [0.5, 1.5], biases in [-0.3, 0.3] (a fresh module has 1 and 0: nothing for an affine to get wrong)."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in module.modules():
            if isinstance(m, torch.nn.GroupNorm):
                m.weight.copy_(torch.rand(m.weight.shape, generator=gen) + 0.5)
                m.bias.copy_(torch.rand(m.bias.shape, generator=gen) * 0.6 - 0.3)
    return module


def module64(module, *args):
    """The float64 copy of a module on the CPU, applied."""
    with torch.no_grad():
        return copy.deepcopy(module).cpu().double()(*(a.double().cpu() for a in args))
