"""What the tests of the heads' dense 3x3 convolutions share (tests/test_head_convs_cpu.py, tests/test_head_convs.py): the two
yardsticks against the float64 ``F.conv2d`` of the same float32 inputs on the CPU, and a numpy restatement of the kernels'
arithmetic (vfa_amd/csrc/vfa_conv.hip, vfa_dense.h) on which the yardsticks are shown to discriminate before a GPU sees them.

(E) elementwise, the raw convolution:  |y - y64| <= gamma_n (|x| conv |w|),  gamma_n = n u / (1 - n u),  u = 2^-24.
    Dense kernel: n = 27 C + 12 -- three products of 9 C terms in any order, 8 u for the two split residuals (2^-23 of each operand,
    twice) and the dropped lo.lo (2^-22), and the epilogue.  Few-output kernel: n = 9 C + 4.  Loose: it catches indexing.
(N) normwise:  ||y - y64|| / ||y64||  <=  4 x the same quantity of the float32 library chain on the CPU, on the same inputs: the
    project's standing convention for float paths.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
EXP = 14            # kExp of vfa_dense.h
EXP_LIMIT = 40      # kExpLim of vfa_split.h
CHUNK, STEP = 32, 16
N_MARGIN = 4.0


def gamma(n):
    return n * U / (1.0 - n * U)


def n_dense(C):
    return 27 * C + 12


def n_few(C):
    return 9 * C + 4


def conv64(x, w, d):
    return F.conv2d(x.double().cpu(), w.double().cpu(), padding=d, dilation=d)


def conv32(x, w, d):
    return F.conv2d(x.float().cpu(), w.float().cpu(), padding=d, dilation=d)


def normwise(y, y64):
    y = torch.as_tensor(y).double().cpu()
    return float((y - y64).norm() / y64.norm())


def check_elementwise(y, x, w, d, n, what=""):
    """(E) -> the largest ratio error / bound (printed before the assertion)."""
    y = torch.as_tensor(y).double().cpu()
    err = (y - conv64(x, w, d)).abs()
    bound = gamma(n) * conv64(x.abs(), w.abs(), d)
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"(E) {what}: max error / bound = {worst:.3g} (n = {n})")
    assert bool((err <= bound).all()), f"(E) {what}: error / bound = {worst:.3g}"
    return worst


def check_normwise(y, y64, y32, what=""):
    """(N) -> (mine, library, ratio), printed before the assertion."""
    mine, lib = normwise(y, y64), normwise(y32, y64)
    print(f"(N) {what}: {mine:.3g} against the library's {lib:.3g}: {mine / lib:.2f} x")
    assert mine <= N_MARGIN * lib, f"(N) {what}: {mine:.3g} > {N_MARGIN} x {lib:.3g}"
    return mine, lib, mine / lib


def inputs(B, C, O, L, W, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, L, W, generator=gen)
    x = x * (1.0 + torch.arange(B, dtype=torch.float32).view(B, 1, 1, 1) * 2.5)  # frames of different scales
    w = torch.randn(O, C, 3, 3, generator=gen) / (9 * C) ** 0.5
    return x, w


def split_exponent(absmax):
    """vfa_split.h: the power of two that brings ``absmax`` into [2^EXP, 2^(EXP + 1)); 0 for zero."""
    if not np.isfinite(absmax) or absmax == 0:
        return 0
    e = int(np.floor(np.log2(float(absmax))))
    return int(np.clip(EXP - e, -EXP_LIMIT, EXP_LIMIT))


def split(v32):
    """Scaled float32 -> (hi, lo) fp16 pieces as float64 arrays."""
    hi = v32.astype(np.float16)
    lo = (v32 - hi.astype(np.float32)).astype(np.float16)
    return hi.astype(np.float64), lo.astype(np.float64)


def emulate_dense(x, w, d, drop_lo=False):
    """The dense kernel's arithmetic: per-frame and per-weight power-of-two scales, the two-piece fp16 split, per 16 k the three
    products x_hi w_lo, x_hi w_hi, x_lo w_hi each added to a float32 accumulator (one rounding per product), chunks of 32 channels,
    taps inside a chunk -> float32 (B, O, L, W).  ``drop_lo``: the hi pieces alone (a plain fp16 product)."""
    xn, wn = x.numpy().astype(np.float32), w.numpy().astype(np.float32)
    B, C, L, W = xn.shape
    O = wn.shape[0]
    ew = split_exponent(np.abs(wn).max())
    wh, wl = split(wn * np.float32(2.0 ** ew))
    out = np.zeros((B, O, L, W), np.float32)
    for b in range(B):
        finite = np.abs(xn[b][np.isfinite(xn[b])])
        ea = split_exponent(finite.max() if finite.size else 0.0)
        xh, xl = split(xn[b] * np.float32(2.0 ** ea))
        xh, xl = (np.pad(p, ((0, 0), (d, d), (d, d))) for p in (xh, xl))
        acc = np.zeros((O, L, W), np.float32)
        for c0 in range(0, C, CHUNK):
            for t in range(9):
                ty, tx = divmod(t, 3)
                for s in range(0, CHUNK, STEP):
                    c = slice(c0 + s, c0 + s + STEP)
                    ah, al = (p[c, ty * d:ty * d + L, tx * d:tx * d + W] for p in (xh, xl))
                    products = [(wh, ah)] if drop_lo else [(wl, ah), (wh, ah), (wh, al)]
                    for wp, ap in products:
                        acc = (acc.astype(np.float64) + np.einsum("oc,clw->olw", wp[:, c, ty, tx], ap)).astype(np.float32)
        out[b] = acc * np.float32(2.0 ** -(ea + ew))
    return torch.from_numpy(out)


def fma32(a, b, c):
    """fmaf on float32 arrays through float64 (the product is exact there)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def emulate_few(x, w, d, affine=None):
    """The few-output kernel's arithmetic: four fmaf chains over a quarter of the channels each (ascending channels, ascending
    taps), merged as (p0 + p1) + (p2 + p3); the prologue relu(a x + b) before the zero padding."""
    xn, wn = x.numpy().astype(np.float32), w.numpy().astype(np.float32)
    B, C, L, W = xn.shape
    O = wn.shape[0]
    if affine is not None:
        a, b = (t.numpy().astype(np.float32) for t in affine)
        xn = np.maximum(fma32(a[:, :, None, None], xn, np.broadcast_to(b[:, :, None, None], xn.shape)), np.float32(0))
    xp = np.pad(xn, ((0, 0), (0, 0), (d, d), (d, d)))
    parts = []
    for p in range(4):
        acc = np.zeros((B, O, L, W), np.float32)
        for c in range(p * C // 4, (p + 1) * C // 4):
            for t in range(9):
                ty, tx = divmod(t, 3)
                tap = xp[:, c, None, ty * d:ty * d + L, tx * d:tx * d + W]
                acc = fma32(np.broadcast_to(tap, acc.shape), np.broadcast_to(wn[None, :, c, ty, tx, None, None], acc.shape), acc)
        parts.append(acc)
    return torch.from_numpy((parts[0] + parts[1]) + (parts[2] + parts[3]))
