"""What the tests of the dense 3x3 convolution's gradients share (tests/test_conv_grad_cpu.py, tests/test_conv_grad.py): the
float64 / float32 references from torch autograd of ``F.conv2d`` on the CPU, the two yardsticks of tests/conv_common.py restated for
the weight gradient, and a numpy restatement of the kernel's arithmetic (vfa_amd/csrc/vfa_conv_grad.hip) on which the yardsticks are
shown to discriminate before a GPU sees them.

    dW[o, c, ty, tx] = sum_b sum_(l, w) g[b, o, l, w] x[b, c, l + (ty - 1) d, w + (tx - 1) d]          (|g| * |x|: the same sum of moduli)

(E) elementwise:  |dW - dW64| <= gamma_n (|g| * |x|),  gamma_n = n u / (1 - n u),  u = 2^-24, with

        n = 3 B L W + 8 + B slabs(L, W)

    derived like ``n_dense``: the sum of an element has B L W terms and the kernel adds three products per term to float32
    accumulators, in any order (3 B L W); 8 u for the split residuals of both operands (2^-23 = 2 u of g and 2 u of x) and the
    dropped lo.lo (2^-22 = 4 u); and one rounding per merge step, of which there are
    B slabs(L, W) -- an upper bound for the kernel's merge, which adds the partials in float64 and rounds once.  The unscaling by
    2^-(eg + ex) is exact.  Computed from the shape, never tuned.  Loose: it catches indexing.
    The bias gradient is a float64 sum rounded once (the float64 additions together are far below one u): n = 2.
(N) normwise:  ||dW - dW64|| / ||dW64||  <=  N_MARGIN = 4 x the same quantity of the float32 autograd chain on the CPU, on the same
    inputs: the project's standing convention for float paths (``conv_common.check_normwise``).
"""
import numpy as np
import torch
import torch.nn.functional as F

import conv_common as cc
from conv_common import N_MARGIN, check_normwise, gamma, normwise, split, split_exponent  # noqa: F401  (shared with the tests)

TILE_ROWS, TILE_COLS, STEP, MAX_SLABS = 4, 32, 16, 16   # vfa_conv.h, vfa_conv_grad.h
N_BIAS = 2


def tiles(L, W):
    return -(-L // TILE_ROWS) * -(-W // TILE_COLS)


def slabs(L, W):
    return min(tiles(L, W), MAX_SLABS)


def slab_tiles(s, L, W):
    """vfa_conv_grad.h: the tiles [n s / slabs, n (s + 1) / slabs) of slab s."""
    n, k = tiles(L, W), slabs(L, W)
    return range(n * s // k, n * (s + 1) // k)


def n_wgrad(B, L, W):
    return 3 * B * L * W + 8 + B * slabs(L, W)


def _autograd(x, w, g, d, bias):
    x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    b = None if bias is None else bias.clone().requires_grad_(True)
    F.conv2d(x, w, b, padding=d, dilation=d).backward(g)
    return x.grad, w.grad, None if b is None else b.grad


def grads64(x, w, g, d, bias=None):
    """(dX, dW, db) from float64 autograd of ``F.conv2d`` on the CPU."""
    return _autograd(x.double().cpu(), w.double().cpu(), g.double().cpu(), d, None if bias is None else bias.double().cpu())


def grads32(x, w, g, d, bias=None):
    """The same from the float32 autograd chain on the CPU."""
    return _autograd(x.float().cpu(), w.float().cpu(), g.float().cpu(), d, None if bias is None else bias.float().cpu())


def wgrad64(g, x, d):
    O, C = g.shape[1], x.shape[1]
    return grads64(x, torch.zeros(O, C, 3, 3), g, d)[1]


def wgrad32(g, x, d):
    O, C = g.shape[1], x.shape[1]
    return grads32(x, torch.zeros(O, C, 3, 3), g, d)[1]


def transposed_flipped(w):
    """The weight of the convolution that gives the input gradient: w'[c, o, ty, tx] = w[o, c, 2 - ty, 2 - tx]."""
    return w.transpose(0, 1).flip(2, 3).contiguous()


def check_elementwise(dw, g, x, d, what=""):
    """(E) of the weight gradient -> the largest ratio error / bound (printed before the assertion)."""
    B, _, L, W = x.shape
    n = n_wgrad(B, L, W)
    err = (torch.as_tensor(dw).double().cpu() - wgrad64(g, x, d)).abs()
    bound = gamma(n) * wgrad64(g.abs(), x.abs(), d)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"(E) {what}: max error / bound = {worst:.3g} (n = {n})")
    assert bool((err <= bound).all()), f"(E) {what}: error / bound = {worst:.3g}"
    return worst


def check_bias_elementwise(db, g, what=""):
    err = (torch.as_tensor(db).double().cpu() - g.double().cpu().sum((0, 2, 3))).abs()
    bound = gamma(N_BIAS) * g.double().cpu().abs().sum((0, 2, 3))
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"(E) {what}: max error / bound = {worst:.3g} (n = {N_BIAS})")
    assert bool((err <= bound).all()), f"(E) {what}: error / bound = {worst:.3g}"
    return worst


def inputs(B, C, O, L, W, seed):
    """x and w of ``conv_common.inputs`` (frames of different scales) and an output gradient whose frames are scaled differently
    again, the other way round."""
    x, w = cc.inputs(B, C, O, L, W, seed)
    gen = torch.Generator().manual_seed(seed + 1000)
    g = torch.randn(B, O, L, W, generator=gen) * 0.01
    g = g * (1.0 + torch.arange(B - 1, -1, -1, dtype=torch.float32).view(B, 1, 1, 1) * 7.0)
    return x, w, g


def emulate_wgrad(g, x, d, variant=None, per_frame=False):
    """The kernel's arithmetic: per frame a power-of-two scale of g and one of x (absmax of the finite values), the two-piece fp16
    split of both; the cells in tiles of 4 rows x 32 columns, a slab a run of tiles (``slab_tiles``); per slab a float32 accumulator
    per tap, to which each step of 16 cells of one tile row adds the three products g_lo x_hi, g_hi x_hi, g_hi x_lo (one rounding
    per product and step); the slab's partial acc * 2^-(eg + ex); the partials added in float64 in ascending (frame, slab) order and
    rounded once -> float32 (O, C, 3, 3).  ``per_frame``: the float32 partials instead, (B, slabs, O, C, 3, 3).
    ``variant``: "hi" the hi pieces alone; "mirror" tap (ty, tx) reads where tap (ty, 2 - tx) should; "edge" pads with the edge
    value instead of zero."""
    gn, xn = g.numpy().astype(np.float32), x.numpy().astype(np.float32)
    B, O, L, W = gn.shape
    C = xn.shape[1]
    S = slabs(L, W)
    tiles_x = -(-W // TILE_COLS)
    partials = np.zeros((B, S, O, C, 3, 3), np.float32)
    for b in range(B):
        scale = []
        for v in (gn[b], xn[b]):
            finite = np.abs(v[np.isfinite(v)])
            scale.append(split_exponent(finite.max() if finite.size else 0.0))
        eg, ex = scale
        gh, gl = split(gn[b] * np.float32(2.0 ** eg))
        xh, xl = split(xn[b] * np.float32(2.0 ** ex))
        xh, xl = (np.pad(p, ((0, 0), (d, d), (d, d)), mode="edge" if variant == "edge" else "constant") for p in (xh, xl))
        for s in range(S):
            acc = np.zeros((3, 3, O, C), np.float32)
            for tile in slab_tiles(s, L, W):
                y0, x0 = tile // tiles_x * TILE_ROWS, tile % tiles_x * TILE_COLS
                for ry in range(TILE_ROWS):
                    for xs in range(x0, x0 + TILE_COLS, STEP):
                        y, x1 = y0 + ry, min(xs + STEP, W)
                        if y >= L or xs >= W:
                            continue          # (cells outside the map are zeros of g: the accumulators do not move)
                        a_hi, a_lo = gh[:, y, xs:x1], gl[:, y, xs:x1]
                        for ty in range(3):
                            for tx in range(3):
                                sx = 2 - tx if variant == "mirror" else tx
                                b_hi, b_lo = (p[:, y + ty * d, xs + sx * d:x1 + sx * d] for p in (xh, xl))
                                products = [(a_hi, b_hi)] if variant == "hi" else [(a_lo, b_hi), (a_hi, b_hi), (a_hi, b_lo)]
                                for ap, bp in products:
                                    acc[ty, tx] = (acc[ty, tx].astype(np.float64) + ap @ bp.T).astype(np.float32)
            partials[b, s] = (acc * np.float32(2.0 ** -(eg + ex))).transpose(2, 3, 0, 1)
    if per_frame:
        return torch.from_numpy(partials)
    return merge_partials(torch.from_numpy(partials))


def merge_partials(partials):
    """The documented merge: (B, slabs, O, C, 3, 3) float32 partials added in float64 in ascending (frame, slab) order, one rounding."""
    total = np.zeros(partials.shape[2:], np.float64)
    for b in range(partials.shape[0]):
        for s in range(partials.shape[1]):
            total = total + partials[b, s].numpy().astype(np.float64)
    return torch.from_numpy(total.astype(np.float32))
