"""What the image front end's tests share: the numpy restatement of the rule ``vfa_amd/csrc/vfa_resize.h`` states (Pillow's
antialiased bilinear resize of 8-bit images, ``ToTensor``, the normalisation), vectorised over pixels, and the records of
``tests/golden/frontend_pil.npz`` (made by ``tests/golden/make_frontend.py`` with Pillow itself).

Per axis, ``n_in`` source and ``n_out`` target length, in Python floats (IEEE doubles, one operation per expression):
``scale = n_in / n_out``, ``fs = max(scale, 1)``, ``support = fs``, ``ksize = int(ceil(support)) * 2 + 1``, ``ss = 1 / fs``; output
index ``xx``: ``center = (xx + 0.5) * scale``, ``xmin = max(int(center - support + 0.5), 0)``, ``n = min(int(center + support + 0.5),
n_in) - xmin``, ``w[x] = tri((x + xmin - center + 0.5) * ss)``, ``ww`` their left-to-right sum, ``k[x] = int(0.5 + w[x] / ww * 2**22)``.
A pass: ``clip((2**21 + sum(pixel * k)) >> 22, 0, 255)`` as a byte; horizontal first, the vertical pass on its bytes; an axis that
keeps its length is skipped."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend_pil.npz")
PRECISION_BITS = 22
MAX_TAPS, MAX_LENGTH = 17, 16384
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)   # VFANet's buffers
FULL = ((1080, 1920), (720, 1280))                         # the workload's own shape
# (input (h, w), output (h, w)): the records of the fixture
SHAPES = (((37, 53), (19, 31)), ((19, 31), (37, 53)), ((64, 48), (64, 20)), ((33, 70), (9, 70)), ((40, 40), (5, 7)), ((7, 5), (40, 41)),
          ((100, 100), (13, 99)))
TENSOR_SHAPES = (0, 4)   # the records that also hold the float32 tensors


def key(shape, name):
    (ih, iw), (oh, ow) = shape
    return f"{ih}x{iw}_{oh}x{ow}_{name}"


def load():
    return np.load(GOLDEN)


def ksize_of(n_in, n_out):
    return int(math.ceil(max(n_in / n_out, 1.0))) * 2 + 1


def coefficients(n_in, n_out):
    """-> (xmin (n_out), n (n_out), k (n_out, ksize) int64, zero behind the taps)."""
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fs
    first, count, k = np.zeros(n_out, np.int64), np.zeros(n_out, np.int64), np.zeros((n_out, ksize), np.int64)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), n_in) - xmin
        w = []
        for x in range(n):
            a = abs((x + xmin - center + 0.5) * ss)
            w.append(1.0 - a if a < 1.0 else 0.0)
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            k[xx, x] = int(0.5 + (v / ww if ww != 0.0 else v) * (1 << PRECISION_BITS))
        first[xx], count[xx] = xmin, n
    return first, count, k


def resize_pass(img, n_out, axis):
    """One pass along ``axis`` of a uint8 array, every other axis vectorised."""
    src = np.moveaxis(img, axis, 0).astype(np.int32)
    first, count, k = coefficients(src.shape[0], n_out)
    acc = np.full((n_out,) + src.shape[1:], 1 << (PRECISION_BITS - 1), np.int32)
    tail = (1,) * (src.ndim - 1)
    for t in range(k.shape[1]):
        at = np.minimum(first + t, src.shape[0] - 1)     # (a tap behind the last has the coefficient 0)
        acc += src[at] * k[:, t].astype(np.int32).reshape(-1, *tail)
    return np.moveaxis(np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8), 0, axis)


def resize(img, size):
    """img (..., H, W, 3) uint8, size (oh, ow) -> (..., oh, ow, 3) uint8."""
    oh, ow = size
    if ow != img.shape[-2]:
        img = resize_pass(img, ow, img.ndim - 2)
    if oh != img.shape[-3]:
        img = resize_pass(img, oh, img.ndim - 3)
    return img


def to_tensor(u8, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
    """(..., H, W, 3) uint8 -> (..., 3, H, W) float32: ``ToTensor`` and ``(x - mean) / std`` as float32 operations of numpy (IEEE)."""
    t = np.moveaxis(u8, -1, -3).astype(np.float32) / np.float32(255.0)
    m = np.asarray(mean, np.float32).reshape(3, 1, 1)
    s = np.asarray(std, np.float32).reshape(3, 1, 1)
    return ((t - m) / s).astype(np.float32)


def frontend(u8, size=None, mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0)):
    return to_tensor(u8 if size is None else resize(u8, size), mean, std)


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
