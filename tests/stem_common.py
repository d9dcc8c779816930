"""What the tests of the trunk's stem share (tests/test_stem_cpu.py, tests/test_stem.py): the yardsticks of tests/conv_common.py for a
7 x 7 stride-2 convolution of three channels, and a numpy restatement of the arithmetic of vfa_amd/csrc/vfa_stem.hip -- the
convolution's one fmaf chain in the kernel's k order, the pooling, the stem and the whole trunk.

(E) elementwise:  |y - y64| <= gamma_n (|x| conv |w|),  n = 147: a float32 sum of 147 products in any order, fused or not.
(N) normwise:  ||y - y64|| / ||y64|| <= 4 x the same quantity of the float32 library chain on the CPU, on the same inputs.
Pooling: one rounding (the fmaf) in front of a maximum, so |out - out64| <= 2 u |out64| against the float64 chain, and the same NaNs.
"""
import numpy as np
import torch
import torch.nn.functional as F

import conv_common as cc
import trunk_common as tc

N_STEM = 147        # kK of vfa_stem.h
MAX_OUT = 64        # kMaxOut
TILE = (4, 32)      # kTileRows, kTileCols: output cells of a tile


def out_size(n):
    return (n - 1) // 2 + 1


def conv(x, w, dtype):
    return F.conv2d(x.to(dtype).cpu(), w.to(dtype).cpu(), stride=2, padding=3)


def check_elementwise(y, x, w, what=""):
    """(E) -> the largest ratio error / bound (printed before the assertion)."""
    y = torch.as_tensor(y).double().cpu()
    err = (y - conv(x, w, torch.float64)).abs()
    bound = cc.gamma(N_STEM) * conv(x.abs(), w.abs(), torch.float64)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"(E) {what}: max error / bound = {worst:.3g} (n = {N_STEM})")
    assert bool((err <= bound).all()), f"(E) {what}: error / bound = {worst:.3g}"
    return worst


def check_both(y, x, w, what=""):
    """(E) and (N) of a raw stem convolution -> the (N) ratio."""
    check_elementwise(y, x, w, what)
    return cc.check_normwise(y, conv(x, w, torch.float64), conv(x, w, torch.float32), what)[2]


def inputs(B, O, L, W, seed):
    """Images of different scales and a (O, 3, 7, 7) weight that is not symmetric in (ky, kx)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, 3, L, W, generator=gen)
    x = x * (1.0 + torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1) * 2.5)
    w = torch.randn(O, 3, 7, 7, generator=gen) / 147 ** 0.5
    return x, w


def emulate_conv(x, w, pad=3, swap=False):
    """The stem kernel's arithmetic: per output ONE float32 fmaf chain over k = (c 7 + ky) 7 + kx ascending, a tap outside the image
    being a zero operand (the padded k = 147 adds 0 * 0) -> float32 (B, O, Lo, Wo).  Two WRONG variants for the yardstick to catch:
    ``pad`` other than 3 (the window starts elsewhere), ``swap`` (ky and kx exchanged on the image side)."""
    xn, wn = x.numpy().astype(np.float32), w.numpy().astype(np.float32)
    B, C, L, W = xn.shape
    O = wn.shape[0]
    Lo, Wo = out_size(L), out_size(W)
    far = 3 + 6                                                     # room for every variant's taps
    xp = np.pad(xn, ((0, 0), (0, 0), (far, far + 1), (far, far + 1)))
    acc = np.zeros((B, O, Lo, Wo), np.float32)
    for c in range(3):
        for ky in range(7):
            for kx in range(7):
                ty, tx = (kx, ky) if swap else (ky, kx)
                y0, x0 = far - pad + ty, far - pad + tx
                tap = xp[:, c, None, y0:y0 + 2 * (Lo - 1) + 1:2, x0:x0 + 2 * (Wo - 1) + 1:2]
                acc = cc.fma32(np.broadcast_to(tap, acc.shape), np.broadcast_to(wn[None, :, c, ky, kx, None, None], acc.shape), acc)
    return torch.from_numpy(acc)


def pool_affine(B, C, seed):
    """a and b of both signs."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, generator=gen), torch.randn(B, C, generator=gen)


def emulate_pool(y, affine, affine_last=False):
    """``vfa_stem_pool_f32``: per tap max(fmaf(a, y, b), 0) in float32 (a NaN stays), then the maximum over the taps inside the map, a NaN
    tap taking the cell.  ``affine_last`` is the WRONG order: the maximum of the raw taps first, the affine and the ReLU after it."""
    yn = y.numpy().astype(np.float32)
    a, b = (np.broadcast_to(t.numpy().astype(np.float32)[:, :, None, None], yn.shape) for t in affine)

    def act(v, a, b):
        t = cc.fma32(a, v, b)
        return np.where(t < 0, np.float32(0), t)
    B, C, L, W = yn.shape
    Lo, Wo = out_size(L), out_size(W)
    taps = yn if affine_last else act(yn, a, b)
    padded = np.full((B, C, L + 3, W + 3), -np.inf, np.float32)     # a tap outside the map never wins and is never a NaN
    padded[:, :, 1:1 + L, 1:1 + W] = taps
    best = np.full((B, C, Lo, Wo), -np.inf, np.float32)
    for ty in range(3):
        for tx in range(3):
            t = padded[:, :, ty:ty + 2 * (Lo - 1) + 1:2, tx:tx + 2 * (Wo - 1) + 1:2]
            best = np.where((t > best) | np.isnan(t), t, best)
    if affine_last:
        best = act(best, a[:, :, :Lo, :Wo], b[:, :, :Lo, :Wo])
    return torch.from_numpy(best.astype(np.float32))


def pool64(y, affine):
    a, b = (t.double()[:, :, None, None] for t in affine)
    return F.max_pool2d(F.relu(a * y.double() + b), 3, stride=2, padding=1)


def check_pool(out, y, affine, what=""):
    """Against the float64 chain: the same NaN cells, and elsewhere within one rounding of the fmaf -> the largest error in units of
    u |out64| (printed before the assertion)."""
    out = torch.as_tensor(out).double().cpu()
    want = pool64(y, affine)
    assert out.shape == want.shape, (out.shape, want.shape)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(out), nan), f"{what}: the NaN cells differ"
    err, scale = (out - want).abs()[~nan], want.abs()[~nan]
    worst = float((err / (cc.U * scale).clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"pool {what}: max error = {worst:.3g} u |out64|")
    assert bool((err <= 2 * cc.U * scale).all()), f"pool {what}: {worst:.3g} u"
    return worst


def emulate_stem(trunk, x):
    """``_Trunk.stem_hip`` restated: the raw convolution, its GroupNorm as an affine, the pooling."""
    y = emulate_conv(x, trunk.conv1.weight.detach())
    return emulate_pool(y, tc.emulate_gn_affine(y, trunk.bn1))


def emulate_trunk(trunk, x):
    """The trunk with both halves on the HIP kernels, restated: ``emulate_stem`` and the blocks of tests/trunk_common.py."""
    with torch.no_grad():
        x = emulate_stem(trunk, x)
        maps = []
        for layer in (trunk.layer1, trunk.layer2, trunk.layer3, trunk.layer4):
            for block in layer:
                x = tc.emulate_block(block, x)
            maps.append(x)
    return maps[1], maps[2], maps[3]
