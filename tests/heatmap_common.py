"""What the heat-map tests share: a numpy restatement of the rules of vfa_amd/csrc/vfa_heat.h (the reference's
``RotationGaussianKernel`` and ``GaussianKernel``, vfa/data/GK.py) in float32 -- the reference's own arithmetic -- or float64, with the
three deviations (arg-max tie -> first, cells outside the map dropped, duplicates count once); the fixtures; the tolerance rule.

THE TOLERANCE RULE of every comparison of a rendered map ``out`` with a reference evaluated twice (``ref32`` from a float32 map,
``ref64`` from a float64 map): ``max |out - ref64| <= 4 * max |ref32 - ref64|`` over EVERY cell -- the reference's own float32 error,
times 4 for the device's exp against numpy's float32 exp and the other summation order of the convolution, the project's rule for the
loss -- and exactly: ``{out == 1} == {ref32 == 1}``, ``ref64 == 0 => out == 0``.  Figures are printed before they are asserted."""
import functools
import math
import os

import numpy as np

from conftest import golden_path

FIXTURES = ("heatmap_mc.npz", "heatmap_wt.npz")
MAX_K = 64
WILDTRACK = 2


@functools.lru_cache(maxsize=None)
def load(name):
    return dict(np.load(golden_path(name), allow_pickle=False))


# ---- the object's cell: vfa_loss.h assign_cell (float32, one rounding per operation) -----------------------------------------------

def cell_of(x, y, world, grid_lw, kind):
    """-> (row, col) or None (outside the map or non-finite)."""
    L, W = grid_lw
    f = np.float32
    with np.errstate(all="ignore"):
        u = f(x) / f(world[0]) * f(L)
        v = f(y) / f(world[1]) * f(W)
    if not (np.isfinite(u) and np.isfinite(v) and abs(u) < 2.0 ** 31 and abs(v) < 2.0 ** 31):
        return None
    cx, cy = int(u), int(v)
    row, col = (cx, cy) if kind == WILDTRACK else (cy, cx)
    if row < 0 or col < 0 or row >= L or col >= W:
        return None
    return row, col


# ---- RGK ---------------------------------------------------------------------------------------------------------------------------

def kernel_k(l, w, alpha=0.01, ratio=8):
    """k of an object (n = k + 1 taps per side), or None where no kernel can be made (centre only)."""
    std_w, std_l = float(w) * alpha, float(l) * alpha
    if not (std_w > 0 and std_l > 0 and max(std_w, std_l) <= 1e6):
        return None
    size = math.ceil(max(std_w, std_l)) * ratio
    return int(size) if 2 <= size <= MAX_K else None


def rotated_kernel(l, w, deg, alpha=0.01, ratio=8, dtype=np.float32):
    """-> (rot (n, n) dtype, branch (n, n) int: 0 skip / 1 nearest / 2 blend, (g_t, g_l)) or None (centre only)."""
    k = kernel_k(l, w, alpha, ratio)
    if k is None or not (abs(float(deg)) <= 1e9):
        return None
    std_w, std_l = float(w) * alpha, float(l) * alpha
    d_l, d_w = dtype(2.0 * (std_l * std_l)), dtype(2.0 * (std_w * std_w))
    if not (np.float32(d_l) > 0 and np.float32(d_w) > 0):
        return None
    n, lo = k + 1, -((k + 1) // 2)
    axis = np.arange(lo, lo + n).astype(dtype)
    xx, yy = axis[None, :], axis[:, None]
    with np.errstate(under="ignore"):
        taps = np.exp((-(xx * xx)) / d_l - (yy * yy) / d_w)
    assert taps.dtype == dtype
    a = float(deg) * math.pi / 180.0
    c, s = np.float64(np.cos(a)), np.float64(np.sin(a))
    i, j = np.meshgrid(np.arange(n, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    half = 0.5 * n
    d0, d1 = i - half, -j + half
    e0, e1 = d0 * c + d1 * s, d0 * (-s) + d1 * c
    f0, f1 = e0 + half, -e1 + half
    g0, g1 = np.floor(f0), np.floor(f1)
    ni, nj, u, v = g0.astype(np.int64), g1.astype(np.int64), f0 - g0, f1 - g1
    skip = (nj >= n) | (ni >= n) | (ni < 1) | (nj < 1) | (i + 1 >= n) | (j + 1 >= n)
    nearest = ~skip & ((ni + 1 >= n) | (nj + 1 >= n))
    ci, cj = np.clip(ni, 0, n - 2), np.clip(nj, 0, n - 2)  # (only read where the blend applies)
    t = taps.astype(np.float64)
    mixed = (1 - u) * (1 - v) * t[ci, cj] + (1 - u) * v * t[ci, cj + 1] + u * (1 - v) * t[ci + 1, cj] + u * v * t[ci + 1, cj + 1]
    rot = mixed.astype(dtype)
    rot[nearest] = taps[np.clip(ni, 0, n - 1), np.clip(nj, 0, n - 1)][nearest]
    rot[skip] = 0
    at = int(np.argmax(rot))  # the first of the maxima in row-major order
    return rot, np.where(skip, 0, np.where(nearest, 1, 2)), (at // n, at % n)


def below_one(dtype):
    return np.nextafter(dtype(1), dtype(0))


def rgk_map(location, dimension, degrees, world, grid_lw, kind=0, alpha=0.01, ratio=8, dtype=np.float32):
    """One frame: location (n, 2|3), dimension (n, 3) = (h, w, l), degrees (n) -> (map (L, W) dtype, number of clipped objects)."""
    L, W = grid_lw
    out, clipped = np.zeros((L, W), dtype), 0
    for loc, dim, deg in zip(location, dimension, degrees):
        at = cell_of(loc[0], loc[1], world, grid_lw, kind)
        if at is None:
            continue
        made = rotated_kernel(dim[2], dim[1], deg, alpha, ratio, dtype)
        if made is None:
            clipped += 1
        else:
            rot, _, (g_t, g_l) = made
            n = rot.shape[0]
            top, left = at[0] - g_t, at[1] - g_l
            r0, r1, q0, q1 = max(0, -top), min(n, L - top), max(0, -left), min(n, W - left)
            if r0 < r1 and q0 < q1:
                window = out[top + r0:top + r1, left + q0:left + q1]
                np.maximum(window, np.minimum(rot[r0:r1, q0:q1], below_one(dtype)), out=window)
    for loc in location:  # (a centre is 1 whatever is pasted over it: after all kernels)
        at = cell_of(loc[0], loc[1], world, grid_lw, kind)
        if at is not None:
            out[at] = 1
    return out, clipped


# ---- GK ----------------------------------------------------------------------------------------------------------------------------

def gk_table(grid_reduce=4, radius=8):
    x = np.arange(-radius, radius + 1, dtype=np.float64)
    return np.exp(-(x[None, :] ** 2 + x[:, None] ** 2) / (2.0 * (8.0 / grid_reduce))).astype(np.float32)


def gk_map(location, world, grid_lw, kind=0, grid_reduce=4, radius=8, dtype=np.float32):
    """One frame.  float32: the float32 table summed in float64 in raster order of the table and rounded once (the kernel's order,
    so its bits); float64: the same sum left in float64."""
    L, W = grid_lw
    occ = np.zeros((L, W), bool)
    for loc in location:
        at = cell_of(loc[0], loc[1], world, grid_lw, kind)
        if at is not None:
            occ[at] = True
    table, r = gk_table(grid_reduce, radius), radius
    padded = np.zeros((L + 2 * r, W + 2 * r), np.float64)
    padded[r:r + L, r:r + W] = occ
    total = np.zeros((L, W), np.float64)
    for i in range(2 * r + 1):
        for j in range(2 * r + 1):
            total += padded[i:i + L, j:j + W] * np.float64(table[i, j])
    out = total.astype(dtype)
    out[occ] = 1
    return out


# ---- the tolerance rule ------------------------------------------------------------------------------------------------------------

def check_map(out, ref32, ref64, what):
    out, ref32, ref64 = np.asarray(out), np.asarray(ref32), np.asarray(ref64, dtype=np.float64)
    assert out.shape == ref32.shape == ref64.shape and out.dtype == np.float32, (what, out.shape, out.dtype)
    e_ref = float(np.abs(ref32.astype(np.float64) - ref64).max())
    err = float(np.abs(out.astype(np.float64) - ref64).max())
    ulps = int(np.count_nonzero(out.view(np.uint32) != ref32.astype(np.float32).view(np.uint32)))
    print(f"{what}: max |out - ref64| {err:.3e}  e_ref = max |ref32 - ref64| {e_ref:.3e}  bound {4 * e_ref:.3e}  "
          f"cells differing from ref32 in a bit {ulps} of {np.count_nonzero(ref32)} non-zero")
    assert np.array_equal(out == 1, ref32 == 1), what
    assert not out[ref64 == 0].any(), what
    assert err <= 4 * e_ref, (what, err, e_ref)
    return err, e_ref


def frames_of(d, tag):
    """The objects of the RGK frames of a fixture (``tag`` = "rgk") -> list of (location (n, 3), dimension (n, 3), degrees (n))."""
    return [(d[f"{tag}_location"][b, :n], d[f"{tag}_dimension"][b, :n], d[f"{tag}_degrees"][b, :n]) for b, n in enumerate(d[f"{tag}_count"])]


def border_objects():
    """(x, y, l, w, degrees) on the fixtures' 24 x 40 map of a 512 x 1024 world: objects the reference raises on -- in the corners, on
    the border rows and columns, outside the map, at a NaN -- with the recorded dimensions and angles (the generator asserts their
    arg-max margins), and one whose kernel is above the limit (l = 900: k = 72)."""
    d = load("heatmap_mc.npz")
    dims = [(float(dim[2]), float(dim[1]), float(deg)) for _, dims_, degs in frames_of(d, "rgk") for dim, deg in zip(dims_, degs)]
    spots = [(0.0, 0.0), (852.0, 0.5), (1.0, 613.0), (853.0, 614.0), (400.0, 0.0), (0.5, 300.0), (853.25, 200.0), (300.0, 614.25),
             (30.0, 40.0), (830.0, 590.0), (-50.0, 100.0), (100.0, 2000.0), (float("nan"), 5.0)]
    out = [(x, y, *dims[(3 * i) % len(dims)]) for i, (x, y) in enumerate(spots)]
    return out + [(426.0, 307.0, 900.0, 100.0, 30.0)]
