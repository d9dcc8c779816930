#!/usr/bin/env python3
"""Generate tests/golden/heatmap_{mc,wt}.npz by RUNNING THE REFERENCE (CPU): its ``RotationGaussianKernel`` and ``GaussianKernel``
(vfa/data/GK.py) on a handful of objects the way its datasets call them (multiviewC.py:124-143), every map twice -- from a float32
map, the reference's own, and from a float64 map (for GK: its table through ``conv2d`` in float64).

Runs only in the build container, where the reference is checked out; nothing of the reference is copied.  ``make_golden.py`` is
imported for what it sets up (the reference on ``sys.path``, the stand-in modules); ``np.int`` is put back before the import, the
reference predates its removal.

Maps are 24 x 40 on a world of 512 x 1024 (every coordinate, dimension and angle below is exact in float32, and ``x * L / world`` is
exact in float32 and in float64, so the reference's float64 cell and the encoder's float32 cell are the same number).  RGK: 3 frames
of 12, 9 and 5 objects, l in 150 .. 300, w in 60 .. 140 (k = 16 or 24), angles 0, 90, 180, -90, 45, 135 and generic ones, objects
far enough from the border that the reference's window stays inside its pad (it raises otherwise) but near enough that the pad cuts
kernels off; frame 1 has two objects in one cell and two overlapping bumps.  GK: 3 frames with objects in the corners, on the border
rows and columns, duplicates and a crowd; ``heatmap_wt.npz`` holds GK frames under Wildtrack's index convention (row from x).
Each object's rotated kernel (as ``bi_rotate`` returned it to the reference's own call) and its arg-max are stored.

Asserted here: no arg-max tie; the runner-up of every rotated kernel more than 1e-5 below its maximum (the centre cannot hinge on an
ulp of exp); the number of cells equal to 1 is the number of distinct object cells; the closed form of the GK table equals the
reference's in every float32 bit.

Usage:  python tests/golden/make_heatmaps.py
"""
import os
import sys

import numpy as np

np.int = int  # (numpy >= 1.24 has no np.int; GK.py:37 uses it)

import make_golden  # noqa: E402,F401  (sys.path, the stand-in modules)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from vfa.data.GK import GaussianKernel, RotationGaussianKernel  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import heatmap_common as hc  # noqa: E402  (cell_of, gk_table: our own restatement, to cross-check the inputs)

WORLD, L, W, K = (512.0, 1024.0), 24, 40, 12
ALPHA, RATIO, GRID_REDUCE, RADIUS = 0.01, 8, 4, 8

# (x, y, w, l, degrees); column = x * 24 / 512 < 40, row = y * 40 / 1024 < 24
RGK_FRAMES = [
    [(100.5, 90.25, 60.0, 150.0, 0.0), (300.0, 130.5, 100.0, 200.0, 90.0), (500.25, 100.0, 140.0, 300.0, 180.0),
     (700.0, 95.5, 80.5, 180.0, -90.0), (120.0, 300.0, 120.0, 250.0, 45.0), (330.5, 310.25, 90.0, 210.5, 135.0),
     (560.0, 290.0, 75.0, 160.0, 30.5), (760.5, 330.0, 110.0, 280.0, -67.25), (90.0, 500.0, 64.0, 300.0, 112.75),
     (350.0, 520.5, 130.0, 240.0, 10.125), (600.25, 505.0, 70.0, 190.0, -150.5), (780.0, 515.0, 100.0, 220.0, 77.0)],
    # objects 0 and 1 in one cell (column 10, row 8); 2 and 3 two cells apart: overlapping bumps
    [(215.0, 210.0, 90.0, 200.0, 20.0), (220.5, 215.5, 60.0, 150.0, -45.0), (450.0, 300.0, 120.0, 260.0, 60.25),
     (490.0, 330.0, 100.0, 230.0, 135.0), (70.0, 70.0, 80.0, 170.0, 45.0), (790.0, 540.0, 140.0, 300.0, -12.5),
     (640.0, 80.0, 66.0, 152.0, 90.0), (100.0, 530.0, 95.0, 205.0, 180.0), (320.0, 450.0, 125.0, 275.0, 0.0)],
    [(426.0, 307.0, 140.0, 300.0, 33.0), (64.5, 52.0, 60.0, 150.0, -135.0), (800.0, 550.0, 100.0, 200.0, 101.5),
     (810.0, 64.0, 70.0, 290.0, 5.5), (52.0, 560.0, 135.0, 155.0, -80.0)],
]
GK_FRAMES = [
    [(0.0, 0.0), (852.0, 0.5), (1.0, 613.0), (853.0, 614.0), (400.0, 0.0), (0.5, 300.0), (426.5, 307.0), (853.25, 200.0), (300.0, 614.25)],
    # a crowd around column 20, row 12 (sums above 1), two objects in one cell, twice
    [(430.0, 310.0), (450.0, 310.0), (430.0, 335.0), (452.0, 336.0), (470.0, 320.0), (431.0, 311.0), (410.0, 300.0), (440.0, 290.0),
     (100.0, 100.0), (101.0, 101.0), (700.0, 500.0), (25.0, 590.0)],
    [(640.0, 128.0)],
]
# Wildtrack: row = x * 24 / 512 < 24, column = y * 40 / 1024 < 40
WT_FRAMES = [
    [(0.0, 0.0), (511.0, 0.5), (1.0, 1023.0), (511.5, 1023.5), (250.0, 0.0), (0.5, 500.0), (256.0, 512.0), (300.25, 1000.0)],
    [(200.0, 400.0), (215.0, 400.0), (200.0, 430.0), (222.0, 428.0), (230.0, 410.0), (201.0, 401.0), (64.0, 64.0), (65.0, 65.0),
     (480.0, 900.0)],
    [],
]


def cell_float64(x, y, wildtrack):
    """(box_cx, box_cy) the way the dataset makes them: float64, column then row."""
    u, v = x * L / WORLD[0], y * W / WORLD[1]
    return (v, u) if wildtrack else (u, v)


def check_inputs(frames, wildtrack):
    for objs in frames:
        for o in objs:
            assert all(float(np.float32(t)) == t for t in o), o
            cx, cy = cell_float64(o[0], o[1], wildtrack)
            assert hc.cell_of(o[0], o[1], WORLD, (L, W), hc.WILDTRACK if wildtrack else 0) == (int(cy), int(cx)), o


def run_rgk(objs, dtype, record):
    rgk = RotationGaussianKernel(save_dir="", alpha=ALPHA, GKRatio=RATIO)
    inner = rgk.bi_rotate

    def recording(array, angle, **kw):
        out = inner(array, angle, **kw)
        record.append(out.copy())
        return out
    rgk.bi_rotate = recording
    heat = np.zeros((L, W), dtype=dtype)
    for x, y, w, l, deg in objs:
        cx, cy = cell_float64(x, y, False)
        heat = rgk.gaussian_kernel_heatmap(heat, cx, cy, l, w, deg, alpha=ALPHA, gaussian_kernel_ratio=RATIO)
    return heat


def run_gk(frames, wildtrack):
    gk = GaussianKernel(save_dir="", grid_reduce=GRID_REDUCE)
    for objs in frames:
        heat = np.zeros((L, W), dtype=np.float32)
        for x, y in objs:
            cx, cy = cell_float64(x, y, wildtrack)
            heat = gk.gaussian_kernel_heatmap(heat, cx, cy)
        gk.add_item(heat)
    occupancy = np.stack(gk.heatmaps, axis=0).copy()
    table = gk.map_kernel.float()
    assert np.array_equal(table[0, 0].numpy().view(np.uint32), hc.gk_table(GRID_REDUCE, RADIUS).view(np.uint32))
    gk.generate()
    ref32 = np.asarray(gk.heatmaps)
    with torch.no_grad():
        ref64 = F.conv2d(torch.from_numpy(occupancy).double()[:, None], table.double(), padding=RADIUS)[:, 0].numpy()
    ref64[occupancy == 1] = 1.0
    for b, objs in enumerate(frames):
        distinct = {hc.cell_of(x, y, WORLD, (L, W), hc.WILDTRACK if wildtrack else 0) for x, y in objs}
        assert int((ref32[b] == 1).sum()) == len(distinct) == int((ref64[b] == 1).sum()), b
    return ref32, ref64


def packed(frames, width):
    out = np.zeros((len(frames), K, width), np.float64)
    for b, objs in enumerate(frames):
        for i, o in enumerate(objs):
            out[b, i] = o
    return out


def gk_entries(frames, wildtrack):
    check_inputs(frames, wildtrack)
    ref32, ref64 = run_gk(frames, wildtrack)
    xy = packed(frames, 2)
    loc = np.zeros((len(frames), K, 3), np.float32)
    loc[:, :, :2] = xy
    return dict(gk_location=loc, gk_count=np.array([len(f) for f in frames], np.int32), gk_ref32=ref32.astype(np.float32), gk_ref64=ref64,
                gk_grid_reduce=GRID_REDUCE, gk_radius=RADIUS)


def main():
    common = dict(world_size=np.array(WORLD), grid_lw=np.array([L, W]), alpha=ALPHA, ratio=RATIO)
    check_inputs(RGK_FRAMES, False)
    n_max = 25
    kernels = np.zeros((len(RGK_FRAMES), K, n_max, n_max), np.float32)
    sizes, centres = np.zeros((len(RGK_FRAMES), K), np.int32), np.zeros((len(RGK_FRAMES), K, 2), np.int32)
    ref32, ref64 = [], []
    for b, objs in enumerate(RGK_FRAMES):
        rec32, rec64 = [], []
        ref32.append(run_rgk(objs, np.float32, rec32))
        ref64.append(run_rgk(objs, np.float64, rec64))
        assert ref32[-1].dtype == np.float32 and ref64[-1].dtype == np.float64
        for i, (r32, r64) in enumerate(zip(rec32, rec64)):
            n = r32.shape[0]
            assert r32.dtype == np.float32 and r32.shape == (n, n) and n <= n_max and n % 2 == 1
            for r in (r32, r64):
                top = np.sort(r.ravel())[-2:]
                assert top[1] - top[0] > 1e-5, ("arg-max margin", b, i, top)   # (no tie, and not within an ulp of exp of one)
            at = int(np.argmax(r32))
            assert at == int(np.argmax(r64)), (b, i)
            kernels[b, i, :n, :n], sizes[b, i], centres[b, i] = r32, n, (at // n, at % n)
        distinct = {hc.cell_of(o[0], o[1], WORLD, (L, W), 0) for o in objs}
        assert int((ref32[-1] == 1).sum()) == len(distinct) == int((ref64[-1] == 1).sum()), b
    assert len({hc.cell_of(o[0], o[1], WORLD, (L, W), 0) for o in RGK_FRAMES[1]}) == len(RGK_FRAMES[1]) - 1
    obj = packed(RGK_FRAMES, 5)
    loc, dim = np.zeros((len(RGK_FRAMES), K, 3), np.float32), np.ones((len(RGK_FRAMES), K, 3), np.float32)
    loc[:, :, :2], dim[:, :, 1], dim[:, :, 2] = obj[:, :, :2], obj[:, :, 2], obj[:, :, 3]
    for b, objs in enumerate(RGK_FRAMES):
        dim[b, len(objs):] = 1.0
    out = dict(common, base="MultiviewC", rgk_location=loc, rgk_dimension=dim, rgk_degrees=obj[:, :, 4].copy(),
               rgk_count=np.array([len(f) for f in RGK_FRAMES], np.int32), rgk_ref32=np.stack(ref32), rgk_ref64=np.stack(ref64),
               rgk_kernels=kernels, rgk_kernel_n=sizes, rgk_centre=centres, **gk_entries(GK_FRAMES, False))
    for fname, entries in (("heatmap_mc.npz", out), ("heatmap_wt.npz", dict(common, base="Wildtrack", **gk_entries(WT_FRAMES, True)))):
        np.savez_compressed(os.path.join(HERE, fname), **entries)
        e = {t: float(np.abs(entries[f"{t}_ref32"] - entries[f"{t}_ref64"]).max()) for t in ("rgk", "gk") if f"{t}_ref32" in entries}
        print(fname, "e_ref = max |ref32 - ref64|", e, "max", {t: float(entries[f"{t}_ref32"].max()) for t in e},
              "size", os.path.getsize(os.path.join(HERE, fname)))


if __name__ == "__main__":
    main()
