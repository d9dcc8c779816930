#!/usr/bin/env python3
"""Geometry-gradient fixtures: what the reference's OWN ``backward()`` leaves in ``calib.grad`` and ``grid.grad``.

Runs only where the reference is importable (the stand-in modules of ``make_golden.py``; nothing of the reference is copied).  Per
case, the feature maps, collapse weights / biases and the probe come from ``tests/geomgrad_common.inputs`` (numpy's fixed-stream
``RandomState``: the fixture keeps the seed and shapes, the tests draw the same tensors again); the calibration matrices and the
ground grid are stored.  ``calib`` and ``grid`` require grad, everything else is frozen; loss = sum(ortho * probe):

  * module level (one ``VFA.forward``, vfa/model/vfa_op.py:61-125);
  * frame level (the camera loop of ``VFANet.forward``, vfa/model/vfanet.py:64-82: three modules per camera, ``f8 + f16 + f32``).

Each is run in fp32 (the reference as it runs) and with the reference cast to float64; both gradients are stored, and their distance
n = max|g32 - g64| / max|g64| is the reference's own rounding noise -- the yardstick of tests/test_geometry_gradients.py.  ``min_area``
is the smallest area (in feature pixels) of a visible box: a sliver (area ~ 1e-3 and below) turns the quotient's rounding into gradient
noise of order one.

Usage:  python tests/golden/make_geom_gradients.py      (writes tests/golden/geomgrad_*.npz)
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (installs the stand-in modules, imports the reference)

import torch  # noqa: E402

import geomgrad_common as gc  # noqa: E402
from vfa_amd.synthetic import look_at_camera, ring_cameras  # noqa: E402

RefVFA, ref_make_grid = mg.RefVFA, mg.ref_make_grid
torch.set_num_threads(4)


def _mods(data, image_size, cube_size, grid_height, C, inp, n_scales):
    args = types.SimpleNamespace(data=data, image_size=tuple(image_size))
    mods = []
    for s in range(n_scales):
        m = RefVFA(channel=C, grid_height=grid_height, cube_size=cube_size, args=args)
        with torch.no_grad():
            m.collapse.weight.copy_(torch.from_numpy(inp["weights"][s]))
            m.collapse.bias.copy_(torch.from_numpy(inp["biases"][s]))
        for p in m.parameters():
            p.requires_grad_(False)
        mods.append(m)
    return mods


def _run(mods, feats, calibs, grid, probe, dtype, capture):
    """sum_cam sum_scale VFA(...) (the camera loop) in `dtype` -> ortho, d calibs, d grid."""
    ms = [m.to(dtype) for m in mods]
    cal = calibs.to(dtype).clone().requires_grad_(True)
    g = grid.to(dtype).clone().requires_grad_(True)
    orig = mg.ref_op.torch.logical_and

    def land(a, b, *r, **k):
        out = orig(a, b, *r, **k)
        capture.append(out.detach().clone())
        return out

    mg.ref_op.torch.logical_and = land
    try:
        ortho = 0
        for cam in range(cal.shape[0]):                                                      # vfanet.py:65
            f = [m(torch.from_numpy(feats[s][cam:cam + 1]).to(dtype), cal[cam], g) for s, m in enumerate(ms)]
            o = f[0]
            for x in f[1:]:
                o = o + x
            ortho = ortho + o                                                                # :79, :82
        (ortho * torch.from_numpy(probe).to(dtype)[None]).sum().backward()
    finally:
        mg.ref_op.torch.logical_and = orig
    return ortho.detach(), cal.grad.detach().clone(), g.grad.detach().clone()


def case(fname, data, image_size, cube_size, grid_height, grid, calibs, C, feat_hws, seed, signed=False, wscale=3.0):
    L, W = grid.shape[1:3]
    nl = len(gc.z_layers(grid_height, cube_size))
    inp = gc.inputs(seed, calibs.shape[0], C, feat_hws, nl, L, W, wscale=wscale, signed=signed)
    mods = _mods(data, image_size, cube_size, grid_height, C, inp, len(feat_hws))
    cap32, cap64 = [], []
    o32, c32, g32 = _run(mods, inp["feats"], calibs, grid, inp["probe"], torch.float32, cap32)
    o64, c64, g64 = _run(mods, inp["feats"], calibs, grid, inp["probe"], torch.float64, cap64)
    for v32, v64 in zip(cap32, cap64):
        assert torch.equal(v32, v64), f"{fname}: fp32 and float64 disagree on the visibility of a box; pick another seed"
    min_area = _min_visible_area(mods[0], calibs, grid, feat_hws)
    active = float((o32 > 0).double().mean())
    vis = float(np.mean([float(v.double().mean()) for v in cap32]))
    noise = {k: float((a.double() - b).abs().max() / b.abs().max()) for k, a, b in (("calib", c32, c64), ("grid", g32, g64))}
    np.savez_compressed(os.path.join(HERE, fname), data=data, image_size=np.array(image_size), cube_size=np.array(cube_size, dtype=np.float64),
                        grid_height=np.array(grid_height), seed=np.array(seed), C=np.array(C), feat_hws=np.array(feat_hws), signed=np.array(signed),
                        wscale=np.array(wscale), calibs=calibs.numpy(), grid=grid[0].numpy(),
                        feat_sum=np.array([float(np.sum(f, dtype=np.float64)) for f in inp["feats"]]),
                        d_calibs=c32.numpy(), d_grid=g32[0].numpy(), d_calibs64=c64.numpy(), d_grid64=g64[0].numpy(),
                        noise_calib=np.array(noise["calib"]), noise_grid=np.array(noise["grid"]), min_area=np.array(min_area),
                        ortho_absmax=np.array(float(o32.abs().max())))
    print(f"{fname}: {calibs.shape[0]} camera(s) x {len(feat_hws)} scale(s), C {C}, nl {nl}, grid {L}x{W}, visible {vis:.2f}, "
          f"{active:.0%} outputs active, smallest visible area {min_area:.2e}; fp32 vs float64 of the reference: calib {noise['calib']:.2e}, "
          f"grid {noise['grid']:.2e}")


def _min_visible_area(m, calibs, grid, feat_hws):
    """Smallest area (feature pixels, the reference's expression vfa_op.py:104-106) of a visible box over cameras and scales."""
    from oracle import torch_reference as ref
    zl = m.z_corners[:, 0, 0, 2].double()
    co = m.corners_offset.reshape(8, 3).double()
    best = np.inf
    for cam in range(calibs.shape[0]):
        for hw in feat_hws:
            st = ref.vfa_stages(torch.zeros(1, 1, *hw, dtype=torch.float32), calibs[cam], grid[0], zl.float(), co.float(), m.args.data,
                                m.args.image_size)
            a, v = st["area"], st["visible"]
            if bool(v.any()):
                best = min(best, float(a[v].min()))
    return best


def main():
    mc = ring_cameras(3, (1950.0, 1950.0, 0.0), 2800.0, 600.0, 900.0, (1280, 720))
    g3 = ref_make_grid((3750, 3750), cube_LW=[250, 375], dataset="MultiviewC").unsqueeze(0)  # (1,15,10,3)
    # ---- C = 256: the shapes of the fused training node (serial kernel at nl = 1, pipelined at nl > 1) and of the unfused path -----
    case("geomgrad_mc_c256_nl1.npz", "MultiviewC", (720, 1280), (18.75, 18.75, 160), 160, g3, mc[1][None], 256, [(12, 20)], 71)
    case("geomgrad_mc_c256_nl5.npz", "MultiviewC", (720, 1280), (18.75, 18.75, 32), 160, g3, mc[1][None], 256, [(12, 20)], 72)
    # ---- the other conversions, multi-layer, small C -----------------------------------------------------------------------------
    gw = ref_make_grid((480, 1440), cube_LW=[32, 60], dataset="Wildtrack").unsqueeze(0)
    wt_c = (480 * 2.5 / 2 - 300.0, 1440 * 2.5 / 2 - 900.0, 0.0)
    wcams = ring_cameras(3, wt_c, 0.45 * 1440 * 2.5, 400.0, 1100.0, (1920, 1080))
    case("geomgrad_wt_s8.npz", "Wildtrack", (1080, 1920), (4, 4, 4), 32, gw, wcams[1][None], 8, [(45, 80)], 73)
    gx = ref_make_grid((640, 1000), cube_LW=[50, 40], dataset="MultiviewX").unsqueeze(0)
    mx_cam = torch.tensor(look_at_camera((-5.0, 8.0, 3.0), (12.0, 8.0, 0.0), 1700.0, (1920, 1080)), dtype=torch.float32)
    case("geomgrad_mx_s16.npz", "MultiviewX", (1080, 1920), (4, 4, 8), 64, gx, mx_cam[None], 8, [(45, 80)], 78)
    # ---- a camera inside the scene: clamped corners, boxes cut by the image border; signed features ---------------------------
    inside = torch.tensor(look_at_camera((1500.0, 1700.0, 250.0), (2600.0, 2300.0, 0.0), 700.0, (1280, 720)), dtype=torch.float32)
    g2 = ref_make_grid((3900, 3900), cube_LW=[150, 175], dataset="MultiviewC").unsqueeze(0)
    case("geomgrad_mc_inside_clamped.npz", "MultiviewC", (720, 1280), (25, 25, 32), 160, g2, inside[None], 4, [(45, 80)], 75, signed=True)
    # ---- the camera loop: two cameras x three scales at C = 256, single-layer grid ----------------------------------------------
    gf = ref_make_grid((3750, 3750), cube_LW=[300, 250], dataset="MultiviewC").unsqueeze(0)
    fcams = torch.as_tensor(np.asarray(ring_cameras(2, (1875.0, 1875.0, 0.0), 2700.0, 600.0, 900.0, (1280, 720))), dtype=torch.float32)
    case("geomgrad_frame_mc_nl1.npz", "MultiviewC", (720, 1280), (18.75, 18.75, 160), 160, gf, fcams, 256, [(12, 20), (6, 10), (3, 5)], 76)


if __name__ == "__main__":
    main()
