#!/usr/bin/env python3
"""Generate tests/golden/det_loss_{mc,mx,wt}.npz by RUNNING THE REFERENCE (CPU): its target encoder (vfa/data/encoder.py
``encode3d`` / ``encode2d``) on a handful of objects and its loss (vfa/model/loss.py ``compute_loss3d`` / ``compute_loss2d``) with
autograd on random head outputs, once in float32 and once with every operand cast to float64.

Runs only in the build container, where the reference is checked out; nothing of the reference is copied.  ``make_golden.py`` is
imported for what it sets up -- the reference on ``sys.path`` and the stand-in modules for cv2 / torchvision; the dataset is a
stand-in namespace with the few attributes the encoder reads, as for the decode fixtures.

Maps are small and not square: a world of 300 x 500 at cube 25 -> L x W = 12 x 20, with each dataset kind's index convention.
Objects: a duplicate cell (the later object must win), the last row and column, angles whose degree value is within one float32 ulp
of an integer, negative angles, angles >= 180 degrees.  Heat-map logits: some saturated at +-15, none within 1e-3 of +-11.5129
(where the clamp switches the gradient off).  The dense rotation target and the rotation logits are stored at the mask rows only
(the loss reads no others).

Usage:  python tests/golden/make_det_loss.py
"""
import math
import os
import types

import numpy as np

import make_golden  # noqa: F401  (sys.path, the stand-in modules; it imports nothing of the loss)
import torch

from vfa.data.encoder import ObjectEncoder
from vfa.model import loss as ref_loss

HERE = os.path.dirname(os.path.abspath(__file__))
WORLD, CUBE, MEAN = (300, 500), (25, 25, 32), np.array([140.0, 60.0, 230.0], dtype=np.float32)
L, W, R, SIGMA = 12, 20, 360, 6
CLAMP_EDGE = math.log((1 - 1e-5) / 1e-5)  # 11.5129


def near_integer_degrees(deg, step):
    """The float32 angle next to radians(deg), ``step`` ulps away: its float32 degree value straddles the integer."""
    a = np.float32(math.radians(deg))
    for _ in range(abs(step)):
        a = np.nextafter(a, np.float32(np.inf if step > 0 else -np.inf))
    return float(a)


def objects_of(base):
    """(x, y) so that every object is inside the map under the kind's convention: MultiviewC / MultiviewX index [y-cell, x-cell]
    with x scaled by L and y by W; Wildtrack indexes [x-cell, y-cell]."""
    if base == "Wildtrack":       # row = x / 300 * 12 < 12, column = y / 500 * 20 < 20
        xy = [(12.5, 30.0), (140.2, 260.7), (143.0, 255.1), (299.0, 499.0), (60.6, 410.3), (201.9, 77.7), (88.8, 333.3),
              (250.1, 12.2), (5.0, 480.0)]
    else:                          # column = x / 300 * 12 < 20, row = y / 500 * 20 < 12
        xy = [(12.5, 30.0), (140.2, 260.7), (143.0, 255.1), (499.0, 299.0), (60.6, 110.3), (401.9, 77.7), (88.8, 233.3),
              (250.1, 12.2), (330.0, 5.0)]
    angles = [near_integer_degrees(30, 0), near_integer_degrees(90, -1), near_integer_degrees(90, +1), near_integer_degrees(135, 0),
              math.radians(-45.5), math.radians(-120.25), math.radians(200.0), math.radians(359.2), math.radians(180.0)]
    rng = np.random.RandomState(7)
    dims = MEAN[None, :] * np.exp(rng.randn(len(xy), 3) * 0.15).astype(np.float32)
    return [types.SimpleNamespace(classname="Cow", location=[x, y, 0.0], dimension=[float(v) for v in d], rotation=a)
            for (x, y), d, a in zip(xy, dims, angles)]


def run_loss(fn, pred, gt, weights, dtype):
    leaves = {k: v.detach().to(dtype).requires_grad_(True) for k, v in pred.items()}
    loss, parts = fn(leaves, {k: v.to(dtype) for k, v in gt.items()}, weights)
    loss.backward()
    return parts, {k: v.grad.numpy() for k, v in leaves.items()}


def main():
    for fname, base, seed in (("det_loss_mc.npz", "MultiviewC", 61), ("det_loss_mx.npz", "MultiviewX", 62),
                              ("det_loss_wt.npz", "Wildtrack", 63)):
        three_d = base == "MultiviewC"
        torch.manual_seed(seed)
        ds = types.SimpleNamespace(base=types.SimpleNamespace(label_names=["Cow"], __name__=base), world_size=WORLD, cube_LWH=CUBE,
                                   classAverage=types.SimpleNamespace(get_mean=lambda name: MEAN))
        enc = ObjectEncoder(ds, angle_range=R, angle_radius=SIGMA)
        objs = objects_of(base)
        grid = torch.zeros(L, W, 3)

        # the dense heat-map target (the dataset precomputes it): bumps around the objects, exactly 1 at their cells
        probe = (enc.encode3d if three_d else enc.encode2d)(objs, torch.zeros(L, W), grid)
        mask = probe["mask"][0, 0] == 1
        rows, cols = torch.nonzero(mask, as_tuple=True)
        yy, xx = torch.meshgrid(torch.arange(L, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
        heat_gt = torch.zeros(L, W)
        for r, c in zip(rows.tolist(), cols.tolist()):
            heat_gt = torch.maximum(heat_gt, torch.exp(-((yy - r) ** 2 + (xx - c) ** 2) / 2.0) * 0.97)
        heat_gt[mask] = 1.0
        assert int((heat_gt == 1).sum()) == int(mask.sum())
        gt = (enc.encode3d if three_d else enc.encode2d)(objs, heat_gt, grid)

        heat = torch.randn(1, 1, L, W) * 3.0 - 1.0
        heat[0, 0, 0, :4] = torch.tensor([15.0, -15.0, 15.0, -15.0])
        heat[0, 0, rows[0], cols[0]] = -15.0   # a saturated positive
        heat[0, 0, rows[1], cols[1]] = 15.0
        assert (torch.abs(torch.abs(heat) - CLAMP_EDGE) > 1e-3).all()
        pred = {"heatmap": heat, "loc_offset": torch.randn(1, L, W, 2)}
        weights = [1.0, 1.0]
        if three_d:
            rot = torch.zeros(1, L, W, R)
            rot[0][mask] = torch.randn(int(mask.sum()), R) * 2.5
            pred.update(dim_offset=torch.randn(1, L, W, 3) * 0.4, rotation=rot)
            weights = [1.0, 1.0, 1.0, 1.0]
        fn = ref_loss.compute_loss3d if three_d else ref_loss.compute_loss2d

        out = dict(base=base, world_size=np.array(WORLD), cube_LWH=np.array(CUBE), dimension_mean=MEAN, grid_lw=np.array([L, W]),
                   angle_range=R, angle_radius=SIGMA, loss_weight=np.array(weights, dtype=np.float32),
                   obj_location=np.array([o.location for o in objs], dtype=np.float32),
                   obj_dimension=np.array([o.dimension for o in objs], dtype=np.float32),
                   obj_rotation=np.array([o.rotation for o in objs], dtype=np.float32),
                   gt_mask=gt["mask"][0, 0].numpy(), gt_heatmap=heat_gt.numpy(), gt_loc_offset=gt["loc_offset"][0].numpy(),
                   heatmap=heat.numpy(), loc_offset=pred["loc_offset"].numpy())
        if three_d:
            out.update(gt_dim_offset=gt["dim_offset"][0].numpy(), gt_rotation_rows=gt["rotation"][0][mask].numpy(),
                       dim_offset=pred["dim_offset"].numpy(), rotation_rows=pred["rotation"][0][mask].numpy())
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            parts, grads = run_loss(fn, pred, gt, weights, dtype)
            for k, v in parts.items():
                out[f"{tag}_{k}"] = np.array(v, dtype=np.float64)
            for k, v in grads.items():
                if k == "rotation":
                    assert not v[0][~mask.numpy()].any()
                    v = v[0][mask.numpy()]
                    k = "rotation_rows"
                out[f"{tag}_grad_{k}"] = v
        np.savez_compressed(os.path.join(HERE, fname), **out)
        print(fname, "positives", int(mask.sum()), "of", len(objs), "objects;",
              {k: float(out["f32_" + k]) for k in ("loss", "loss_heatmap", "loss_pos")},
              "size", os.path.getsize(os.path.join(HERE, fname)))


if __name__ == "__main__":
    main()
